"""CPU-only: which kernel a call runs (carma_pack_amd/csrc/carma_shape_plan.h: the series flags, the plans of the batched
log-density, the sampler's family, the row and the ladder sampler's plans) through the stand-alone program tests/shape/plan_main.cpp,
built and run here WITHOUT sanitizers (a sanitizer build of it is a matter for the command line).  (a) every plan equals the
restatement tests/shape_plan_ref.py field for field on a sweep over every threshold; (b) literal cases, written out from the
launchers at 256 CUs and asserted on the program's output alone, so that the restatement cannot share a misreading with the header;
(c) the series flags of the series the other tests build."""
import functools
import os
import subprocess

import numpy as np
import pytest

import shape_plan_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "carma_pack_amd", "csrc")
PLAN_H = os.path.join(CSRC, "carma_shape_plan.h")
MAIN_SRC = os.path.join(HERE, "shape", "plan_main.cpp")
MAIN_EXE = os.path.join(HERE, "shape", "plan_main")
DEPS = [MAIN_SRC, PLAN_H, os.path.join(CSRC, "carma_types.h")]

OK2, WIN_OK, SMALL, REPDT = ref.SERIES_WINDOW2_OK, ref.SERIES_WINDOW_OK, ref.SERIES_WINDOW2_SMALL, ref.SERIES_REPEATED_DT
RING3L = 43584        # Pipe3LGeom<2>::BYTES: (3 + 2) x 16 x 33 + 2 x 33 + 2 + 16 entries of 16 bytes
RING = 33280          # RingGeom<2>::BYTES: 2 x 16 x 64 + 2 x 16 entries of 16 bytes


@functools.lru_cache(None)
def build_main():
    if not os.path.exists(MAIN_EXE) or any(os.path.getmtime(d) > os.path.getmtime(MAIN_EXE) for d in DEPS):
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", MAIN_EXE, MAIN_SRC], check=True, timeout=300)
    return MAIN_EXE


def run(lines):
    """cases, one per line -> the program's lines"""
    r = subprocess.run([build_main()], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = r.stdout.splitlines()
    assert len(out) == len(lines)
    return out


def same(lines, want):
    """the program's line of every case equals the restatement's: every field, and the name"""
    got = run(lines)
    bad = [(c, g, w) for c, g, w in zip(lines, got, want) if g != w]
    assert not bad, "%d of %d differ; the first: case %r program %r restatement %r" % ((len(bad), len(lines)) + bad[0])


def test_the_header_needs_no_hip():
    """carma_shape_plan.h includes the standard library and carma_types.h only: a plain C++ compiler takes it on its own"""
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-x", "c++", PLAN_H], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]
    text = open(PLAN_H).read() + open(os.path.join(CSRC, "carma_types.h")).read()
    assert "#include <hip" not in text and "getenv" not in text and "static std::atomic" not in text


# ---- (a) the sweep ------------------------------------------------------------------------------------------------------------
CUS = (256, 64, 304)
NS = (7, 8, 15, 16, 31, 32, 63, 64, 1024, 1025, 5000, 5001)


def b_values(cus):
    """every threshold of the log-density plans in evaluations, - 1, itself and + 1: k x #CUs for every factor the launchers use
    (2: one two-sided workgroup per CU, 4: one row workgroup, 6 and 12: three; 12 / 16 / 32: lpc_min; 48: the CAR(1) scan; 64, 128,
    192: lpc_max and the unrolled instance; 96 and 112: lane_min) and 256 / 512 / 2048 waves of 8, 16 and 32 evaluations"""
    th = [k * cus for k in (2, 4, 6, 12, 16, 32, 48, 64, 96, 112, 128, 192)] + [w * e for w in (256, 512, 2048) for e in (8, 16, 32)]
    return sorted({b for t in th for b in (t - 1, t, t + 1)} | {1, 2})


def ld_case(p, B, n, flags, cus, lpc, sw):
    return "ld %d %d %d %d %d %d %s" % (p, B, n, flags, cus, lpc, ref.sw_words(sw))


def test_logdens_sweep():
    """p = 2 ... 7 x every threshold +- 1 at three CU counts x the series lengths at which a kernel drops out x all 16 flag words x
    1, 2, 3 resident lpc workgroups; no switch set"""
    cases = [(p, B, n, fl, cus, lpc) for p in range(2, 8) for cus in CUS for B in b_values(cus) for n in NS for fl in range(16) for lpc in (1, 2, 3)]
    u = ref.UNSET
    same([ld_case(*c, u) for c in cases], [ref.ld_line(ref.logdens(*c, u)) for c in cases])


# each switch at 0 and at a value (unset: the sweep above); lpc_rot and the sampler's switches do not move the shape, only their field
LD_SWITCHES = [("win_rows", 0), ("win_rows", 300), ("win2_evals", 0), ("win2_evals", 5000), ("p3l_rows", 0), ("p3l_rows", 100), ("lane_min", 0),
               ("lane_min", 9000), ("lpc_min", 0), ("lpc_min", 2000), ("lpc_max", 0), ("lpc_max", 20000), ("lpc_rot", 0), ("lpc_rot", 0x0102),
               ("p3l_rows", -3), ("pt_row_win", 2), ("pt_plain", 1)]


@pytest.mark.parametrize("name, value", LD_SWITCHES)
def test_logdens_sweep_with_a_switch(name, value):
    sw = ref.switches(**{name: value})
    cases = [(p, B, n, fl, cus, 2) for p in range(2, 8) for cus in CUS for B in b_values(cus) for n in (15, 16, 1024, 5001) for fl in range(16)]
    same([ld_case(*c, sw) for c in cases], [ref.ld_line(ref.logdens(*c, sw)) for c in cases])


def test_car1_sweep():
    sws = [ref.UNSET, ref.switches(car1_scan_max=0), ref.switches(car1_scan_max=1000), ref.switches(car1_scan_max=-1)]
    cases = [(B, n, cus, sw) for cus in CUS for B in b_values(cus) for n in NS for sw in sws]
    same(["car1 %d %d %d %s" % (B, n, cus, ref.sw_words(sw)) for B, n, cus, sw in cases], [ref.ld_line(ref.logdens_car1(*c)) for c in cases])


def r_values(T, cus):
    """ladder counts at which the sampler's choices turn, for T temperatures: the grids of one, two, three workgroups per CU in
    the two-sided and the four-chain form, the lane thresholds (4 x #CUs ladder waves; 12, 16, 48, 64 x #CUs chains)"""
    th = [k * cus // w for k in (1, 2, 3) for w in ((T + 1) // 2, (T + 3) // 4)] + [k * cus // T for k in (12, 16, 48, 64)]
    th += [4 * cus // w for w in (1, 2, 4, 8)] + [cus]
    return sorted({r for t in th for r in (t - 1, t, t + 1) if r >= 1} | {1, 8, 16})


def test_sampler_family_sweep():
    """p = 1 ... 7; T around the 64 of the lane kernel; every forced kernel; the lane override; row occupancies 0 ... 4 and its switch"""
    sws = [ref.UNSET, ref.switches(pt_row_wgs_per_cu=0), ref.switches(pt_row_wgs_per_cu=2)]
    cases = [(p, T, R, n, cus, occ, force, lm, sw) for p in range(1, 8) for T in (1, 4, 10, 16, 64, 65) for cus in CUS for R in r_values(T, cus)
             for n in (31, 32, 63, 64) for occ in (0, 1, 3, 4)
             for force, lm in ((None, None), (None, 0), (None, 4096), ("ladder", None), ("row", None), ("lane", None), ("lane", 10 ** 9))
             for sw in (sws if occ == 3 and force is None else sws[:1])]
    lines = ["fam %d %d %d %d %d %d %d %s %s" % (p, T, R, n, cus, occ, ref.FORCE[force], "u" if lm is None else lm, ref.sw_words(sw))
             for p, T, R, n, cus, occ, force, lm, sw in cases]
    same(lines, ["fam %d %d" % (ref.family(*c), ref.row_capacity(c[1], c[3], c[4], c[5], c[8])) for c in cases])


ROW_SWITCHES = [ref.UNSET] + [ref.switches(**{k: v}) for k, v in (("pt_row_win", 0), ("pt_row_win", 1), ("pt_row_win", 2), ("pt_row_rot", 0), ("pt_row_rot", 0x1234),
                                                                    ("pt_row_xcd_map", 0), ("pt_row_xcd_map", 4), ("win_rows", 0))]


def row_case(R, T, Tg, n, fl, cus, sw):
    return "row %d %d %d %d %d %d %d %s" % (R, T, Tg, n, fl, cus, ref.row_lds(RING3L, Tg, n), ref.sw_words(sw))


def test_row_sampler_sweep():
    """whole and sharded ladders (T of T_global), every word of the three window flags, series around 32, 1024 and the LDS's ~4800 data"""
    cases = [(R, T, Tg, n, fl, cus, sw) for T, Tg in ((1, 1), (4, 4), (10, 10), (16, 16), (4, 16), (8, 16), (64, 64)) for cus in CUS
             for R in r_values(Tg, cus) for n in (31, 32, 1024, 1025, 4000, 5000) for fl in (0, 2, 4, 6, 8, 10, 12, 14, 15) for sw in ROW_SWITCHES]
    want = []
    for c in cases:
        pl = ref.row(c[0], c[1], c[2], c[3], c[4], c[5], ref.row_lds(RING3L, c[2], c[3]), c[6])
        want.append("row " + " ".join(str(int(pl[k])) for k in ref.ROW_FIELDS))
    same([row_case(*c) for c in cases], want)


def test_ladder_sampler_sweep():
    sws = [ref.UNSET, ref.switches(pt_plain=0), ref.switches(pt_plain=1)]
    cases = [(p, 4 if p == 1 else 3 + p + q, T, R, n, cus, RING, sw) for p in range(1, 8) for q in ((0,) if p == 1 else (0, p - 1))
             for T in (1, 8, 16, 17, 32, 33, 64, 65, 128, 256) for cus in CUS for R in (1, cus, cus + 1) for n in (31, 32) for sw in sws]
    lines = ["lad %d %d %d %d %d %d %d %s" % (c[:7] + (ref.sw_words(c[7]),)) for c in cases]
    want = []
    for c in cases:
        pl = ref.ladder(*c)
        want.append("lad " + " ".join(str(int(pl[k])) for k in ref.LAD_FIELDS))
    same(lines, want)


# ---- (b) literal cases, 256 CUs -----------------------------------------------------------------------------------------------
SHAPES = {"P3L": 0, "PC": 1, "PLAIN": 2, "LANE": 3, "LPC": 4, "WIN": 5, "WIN2": 6, "CAR1_SCAN": 7, "CAR1_LANE": 8}


def ld(p, B, n=270, flags=OK2 | WIN_OK, cus=256, lpc=1, **sw):
    f = run([ld_case(p, B, n, flags, cus, lpc, ref.switches(**sw))])[0].split()
    d = dict(zip(ref.LD_FIELDS, map(int, f[1:-1])))
    d["name"] = f[-1]
    return d


def instance(pl):
    """the instantiation a plan launches, as the launcher's switch names it"""
    s, p = pl["shape"], pl["p"]
    if s == SHAPES["WIN2"]:
        if not pl["sl"]:
            return "w2<%d,false,false>" % p
        if not pl["ho"]:
            return "w2<%d,false>" % p
        return "w2<%d,true,true,true>" % p if pl["fold"] else "w2<%d,true>" % p
    if s == SHAPES["LPC"]:
        return "lpc<%d,3,true>" % p if pl["repeated_dt"] else ("lpc<%d,3,false,true>" % p if pl["unrolled"] else "lpc<%d,3>" % p)
    if s == SHAPES["PC"]:
        return "pc<%d,%d,%d>" % (p, pl["G"], pl["pairs"])
    if s == SHAPES["PLAIN"]:
        return "plain<%d,%d,%d>" % (p, pl["G"], pl["waves"])
    return {SHAPES["P3L"]: "p3l", SHAPES["WIN"]: "w", SHAPES["LANE"]: "lane"}[s]


@pytest.mark.parametrize("B, lpc, want", [(512, 1, "w2<5,false>"), (513, 1, "w2<5,true,true,true>"), (1024, 1, "w2<5,true,true,true>"), (1025, 1, "w2<5,true>"),
                                          (1536, 1, "w2<5,true>"), (1537, 1, "p3l"), (3072, 1, "p3l"), (3073, 1, "pc<5,8,2>"), (4096, 1, "pc<5,8,2>"),
                                          (4097, 1, "lpc<5,3,false,true>"), (16384, 1, "lpc<5,3,false,true>"), (16385, 2, "lpc<5,3>"),
                                          (32768, 2, "lpc<5,3>"), (32769, 2, "lane"), (32769, 3, "lpc<5,3>")])
def test_instance_by_evaluation_count(B, lpc, want):
    """p = 5, n = 270, a series that suits both window pipelines, 256 CUs"""
    pl = ld(5, B, lpc=lpc)
    assert instance(pl) == want
    grids = {"w2": ((B + 1) // 2, 256), "p3": ((B + 3) // 4, 256), "pc": ((B + 15) // 16, 256), "lp": ((B + 63) // 64, 256), "la": ((B + 63) // 64, 64)}
    assert (pl["grid"], pl["block"]) == grids[want[:2]]


def test_names_are_the_family():
    assert ld(5, 512)["name"] == ld(5, 1024)["name"] == ld(5, 1536)["name"] == "k_logdens_carma_w2<5>"
    assert ld(5, 4097)["name"] == ld(5, 16385, lpc=2)["name"] == "k_logdens_carma_lpc<5,3>"
    assert ld(5, 4097, flags=REPDT)["name"] == "k_logdens_carma_lpc<5,3,true>" and instance(ld(5, 4097, flags=REPDT)) == "lpc<5,3,true>"
    assert ld(5, 1537)["name"] == "k_logdens_carma_p3l<5>" and ld(5, 4096)["name"] == "k_logdens_carma_pc<5,8,2>"
    assert ld(5, 2048, flags=0, p3l_rows=0)["name"] == "k_logdens_carma_pc<5,8,1>"
    assert ld(5, 40000)["name"] == "k_logdens_carma_lane<5>" and ld(5, 40000, flags=REPDT)["name"] == "k_logdens_carma_lane<5,true>"
    assert ld(4, 1024, flags=WIN_OK)["name"] == "k_logdens_carma_w<4>"
    assert ld(7, 16385)["name"] == "k_logdens_carma<7,8,4>" and ld(7, 16385, flags=REPDT)["name"] == "k_logdens_carma<7,8,4,true>"
    assert ld(2, 64, n=7)["name"] == "k_logdens_carma<2,2,1>"
    assert run(["car1 100 270 256 " + ref.sw_words(ref.UNSET)])[0].split()[-1] == "k_logdens_car1"


def test_other_logdens_cases():
    for p in (3, 4, 6):
        assert instance(ld(p, 1024)) == "w2<%d,true>" % p and not ld(p, 1024)["fold"]      # never the folded instance
    assert instance(ld(7, 1024)) == "w2<7,true,true,true>"
    for B in (2, 512, 513, 1024, 1536):
        assert instance(ld(5, B, n=5001)) == "w2<5,false,false>"                            # the series no longer fits the LDS
    assert ld(5, 512, n=15)["shape"] != SHAPES["WIN2"] and ld(5, 512, n=16)["shape"] == SHAPES["WIN2"]
    assert ld(5, 512, flags=SMALL)["shape"] == SHAPES["WIN2"] and ld(5, 513, flags=SMALL)["shape"] == SHAPES["P3L"]
    for B in (2, 512, 1024, 1536):                                                           # WIN_ROWS = 0: no window kernel of either kind
        assert ld(5, B, win_rows=0)["shape"] == SHAPES["P3L"]
    assert ld(5, 1024, flags=0)["shape"] == SHAPES["P3L"]
    assert ld(5, 1024, flags=0, win_rows=256)["shape"] == SHAPES["WIN2"]                     # any other value lifts the series criterion
    assert ld(5, 1024, flags=0, win_rows=256, win2_evals=0)["shape"] == SHAPES["WIN"]
    assert ld(5, 1024, win2_evals=0)["shape"] == SHAPES["WIN"] and ld(5, 1025, win2_evals=0)["shape"] == SHAPES["P3L"]
    for B in (16385, 24576, 28671):                                                          # p = 7, one lpc workgroup per CU
        assert instance(ld(7, B)) == "plain<7,8,4>"
    assert instance(ld(7, 28672)) == "lane" and instance(ld(7, 16384)) == "lpc<7,3,false,true>"


@pytest.mark.parametrize("B, n, scan", [(12288, 64, True), (12288, 270, True), (12289, 270, False), (12288, 63, False), (1, 64, True), (1, 63, False)])
def test_car1_scan_or_lane(B, n, scan):
    f = run(["car1 %d %d 256 %s" % (B, n, ref.sw_words(ref.UNSET))])[0].split()
    assert int(f[1]) == (SHAPES["CAR1_SCAN"] if scan else SHAPES["CAR1_LANE"])
    assert (int(f[12]), int(f[13])) == ((B, 64) if scan else ((B + 63) // 64, 64))


def fam(p, T, R, n=270, occ=3, force=None, lane_min=None, cus=256, **sw):
    f = run(["fam %d %d %d %d %d %d %d %s %s" % (p, T, R, n, cus, occ, ref.FORCE[force], "u" if lane_min is None else lane_min,
                                                 ref.sw_words(ref.switches(**sw)))])[0].split()
    return ("ladder", "row", "lane")[int(f[1])]


def row(R, T=16, Tg=None, n=270, flags=OK2 | WIN_OK, cus=256, **sw):
    f = run([row_case(R, T, T if Tg is None else Tg, n, flags, cus, ref.switches(**sw))])[0].split()
    return dict(zip(ref.ROW_FIELDS, map(int, f[1:])))


def test_sampler_cases():
    """T = 16, p = 5, n = 270, three row workgroups per CU"""
    assert fam(5, 16, 64) == "row"
    pl = row(64)
    assert pl["two"] and pl["ho"] and pl["sl"] and (pl["wpl"], pl["grid"], pl["minw"], pl["pipeline"]) == (8, 512, 2, 2) and pl["cooperative"]
    assert ref.row_instance(5, pl) == "k_pt_row<5,2,true,true,true>"
    assert fam(5, 16, 65) == "row"
    pl = row(65)
    assert ref.row_instance(5, pl) == "k_pt_row<5,2>" and (pl["wpl"], pl["grid"], pl["pipeline"]) == (4, 260, 0) and pl["cooperative"]
    assert row(128)["minw"] == 2 and row(129)["minw"] == 3 and ref.row_instance(5, row(129)) == "k_pt_row<5,3>"
    assert fam(5, 16, 192) == "row" and all(fam(5, 16, R) == "ladder" for R in (193, 200, 256)) and fam(5, 16, 257) == "lane"
    pl = row(1, T=10)
    assert pl["two"] and not pl["ho"] and pl["wpl"] == 5 and pl["cooperative"] and ref.row_instance(5, pl) == "k_pt_row<5,2,true,true,false>"
    assert not row(1, T=2)["cooperative"] and row(1, T=2)["wpl"] == 1 and row(1, T=2)["rot"] == 0x36D2 and row(1, T=3)["cooperative"]
    assert row(1, T=4, pt_row_win=0)["wpl"] == 1 and not row(1, T=4, pt_row_win=0)["cooperative"]
    pl = row(64, n=1025)
    assert pl["two"] and not pl["sl"] and ref.row_instance(5, pl) == "k_pt_row<5,2,true,true,false,false>"
    assert row(32, n=1025)["sl"] and row(32, n=4000)["sl"] and not row(32, n=5000)["sl"] and not row(33, n=1025)["sl"]      # the LDS holds ~4800 data
    assert [row(16, pt_row_win=w)["pipeline"] for w in (0, 1, 2)] == [0, 1, 2] and [row(65, pt_row_win=w)["pipeline"] for w in (0, 1, 2)] == [0, 1, 1]
    assert row(64, flags=WIN_OK)["pipeline"] == 1 and row(65, flags=WIN_OK)["pipeline"] == 0 and row(64, flags=0)["pipeline"] == 0
    assert row(32, flags=SMALL)["pipeline"] == 2 and row(33, flags=SMALL)["pipeline"] == 0
    assert row(8, T=4, Tg=16)["pipeline"] == 2 and row(8, T=4, Tg=16)["wpl"] == 2 and row(65, T=4, Tg=16)["pipeline"] == 0     # a sharded ladder decides from T_global
    assert row(64)["xcd_map"] == 8 and row(63)["xcd_map"] == 1 and row(64)["rot"] == 0xB14E


def test_forced_sampler_kernels():
    assert fam(5, 16, 64, force="ladder") == "ladder" and fam(5, 16, 64, force="lane") == "lane" and fam(5, 16, 64, force="row") == "row"
    assert fam(5, 16, 257, force="row") == "ladder" and fam(5, 16, 257, force="ladder") == "ladder"   # row only where the grid is resident
    assert fam(5, 16, 1024, force="row") == "ladder"
    assert fam(5, 65, 1, force="lane") == "row" and fam(5, 65, 400, force="lane") == "ladder"         # T = 65: lane is refused
    assert fam(5, 16, 64, occ=0) == "ladder" and fam(5, 16, 64, n=31) == "ladder"
    assert fam(5, 16, 64, lane_min=1024) == "lane" and fam(5, 16, 64, lane_min=1025) == "row" and fam(5, 16, 1024, lane_min=10 ** 6) == "ladder"
    assert fam(5, 16, 129, pt_row_wgs_per_cu=2) == "ladder" and fam(5, 16, 128, pt_row_wgs_per_cu=2) == "row"


@pytest.mark.parametrize("nchain, n, want", [(63, 64, "ladder"), (64, 64, "lane"), (12288, 64, "lane"), (12289, 64, "ladder"), (16384, 64, "ladder"),
                                             (16385, 64, "lane"), (63, 63, "ladder"), (64, 63, "ladder"), (12288, 63, "ladder"), (12289, 63, "ladder"),
                                             (16384, 63, "ladder"), (16385, 63, "ladder")])
def test_car1_sampler(nchain, n, want):
    """CAR(1): one chain per lane from 64 chains on 64 data, but for 48 ... 64 x #CUs chains; never the row sampler"""
    assert fam(1, 1, nchain, n=n) == want


# ---- (c) series flags ----------------------------------------------------------------------------------------------------------
def flags_of(t, p, max_freq=None):
    t = np.asarray(t, dtype=float)
    max_freq = 1.0 / np.min(np.diff(t)) if max_freq is None else max_freq
    got = int(run(["flags %d %r %d %s" % (p, float(max_freq), t.size, " ".join(repr(float(v)) for v in t))])[0].split()[1])
    assert got == ref.series_flags(t, p, float(max_freq))
    return got


def test_series_flags():
    g = np.load(os.path.join(HERE, "golden", "carma53_readme.npz"))
    t = g["t"]
    for p in range(2, 8):
        assert flags_of(t, p) & OK2 and flags_of(t, p) & SMALL
    k = 100                                                   # one close pair of data: max_freq x 100 (tests/test_gpu_window_pipeline.py)
    close = np.insert(t, k + 1, t[k] + 0.01)
    for p in range(2, 8):
        assert not flags_of(close, p) & (OK2 | SMALL)
    reg = np.arange(90.0) * 0.75                              # a regular cadence (tests/test_gpu_mkalman.py)
    for p in (1, 5):
        assert flags_of(reg, p) & REPDT and not flags_of(t, p) & REPDT
    assert flags_of(reg, 1) == REPDT and flags_of(t, 1) == 0  # CAR(1) has no window pipeline
    assert flags_of(reg[:8], 5) & REPDT == 0                  # too short to count
    d = np.loadtxt(os.path.join(HERE, "golden", "ogle_lmc_lpv_00007.dat"))
    for p in (2, 6, 7):
        assert flags_of(np.unique(d[:, 0]), p) & OK2
