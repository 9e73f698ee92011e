"""Which kernel a call runs, restated in Python from the launchers as they stood before carma_shape_plan.h (logdens_shape,
launch_logdens_p and launch_logdens_car1 of carma_kernels.hip; launch_pt_p, pt_row_capacity and launch_pt_row_p of carma_pt.hip; the
sampler-family block of carma_pt_create; the series flags of carma_ctx_create).  tests/test_shape_plan_cpu.py holds the header to
it field for field, tests/test_gpu_shape_plan.py the library's answers on a device.

A switch nobody set is None.  SW_NAMES is the order of ShapeSwitches and of tests/shape/plan_main.cpp's input."""
SERIES_REPEATED_DT, SERIES_WINDOW_OK, SERIES_WINDOW2_OK, SERIES_WINDOW2_SMALL = 1, 2, 4, 8
SW_NAMES = ("win_rows", "win2_evals", "pt_row_win", "p3l_rows", "lane_min", "lpc_min", "lpc_max", "lpc_rot", "car1_scan_max",
            "pt_row_wgs_per_cu", "pt_row_rot", "pt_row_xcd_map", "pt_plain")
UNSET = dict.fromkeys(SW_NAMES)
# LdShape, PtFamily and PtForce as the header numbers them
P3L, PC, PLAIN, LANE, LPC, WIN, WIN2, CAR1_SCAN, CAR1_LANE = range(9)
LADDER, ROW, LANE_FAMILY = 0, 1, 2
FORCE = {None: 0, "ladder": 1, "row": 2, "lane": 3}
W2_MAX_N = 5000
PT_DMAX = 16


def switches(**kw):
    sw = dict(UNSET)
    for k, v in kw.items():
        assert k in sw
        sw[k] = v
    return sw


def group_of(p):
    return 2 if p <= 2 else (4 if p <= 4 else 8)


def _nonneg(v, default):
    """the switches whose "unset" read as -1: any negative value is the default"""
    return v if v is not None and v >= 0 else default


# ---- series flags (carma_ctx_create) -------------------------------------------------------------------------------------------
def series_flags(t, p, max_freq):
    t = [float(v) for v in t]
    n = len(t)
    dt = [0.0] + [t[k] - t[k - 1] for k in range(1, n)]
    rep = sum(dt[k] == dt[k - 1] for k in range(2, n))
    flags = SERIES_REPEATED_DT if n > 8 and 4 * rep >= n else 0
    if p < 2:
        return flags
    ND = 16 - p
    wmin = 0.5 * 600.0 / (6.283185307179586 * max_freq)
    spans = [t[k + ND - 1] - t[k] for k in range(0, n - ND + 1)]
    over = sum(s > wmin for s in spans)
    if len(spans) > 0 and 10 * over <= len(spans):
        flags |= SERIES_WINDOW_OK
    chunks, k = 0, 0
    while k < n:
        j = k
        while j + 1 < n and j + 1 - k < ND and t[j + 1] - t[k] <= wmin:
            j += 1
        k = j + 1
        chunks += 1
    r = chunks / ((n + ND - 1) // ND)
    if r <= 2.0:
        flags |= SERIES_WINDOW2_OK
    if r <= 3.5:
        flags |= SERIES_WINDOW2_SMALL
    return flags


# ---- batched log-density -------------------------------------------------------------------------------------------------------
def lpc_min_evals(p, cus, sw):
    if sw["lpc_min"] is not None and sw["lpc_min"] >= 0:
        return sw["lpc_min"]
    return 12 * cus if p <= 3 else (16 * cus if p == 5 else 32 * cus)


def lane_min_evals(p, cus, sw):
    if sw["lane_min"] is not None and sw["lane_min"] >= 0:
        return sw["lane_min"]
    return 112 * cus if p == 7 else 64 * 4 * cus * 3 // 8


def logdens(p, B, n, flags, cus, lpc_blocks, sw=UNSET):
    """the plan of B evaluations at order p >= 2 as a dict of every field of LdPlan, and its name"""
    G = group_of(p)
    EPW = 64 // G
    waves, rows = (B + EPW - 1) // EPW, (B + 3) // 4
    rep = bool(flags & SERIES_REPEATED_DT)
    pl = dict(shape=None, p=p, G=G, repeated_dt=rep, sl=False, ho=False, fold=False, unrolled=False, pairs=0, waves=0, rot=0, grid=0, block=0)
    win_max_rows = sw["win_rows"] if sw["win_rows"] is not None else cus
    win2_max_evals = sw["win2_evals"] if sw["win2_evals"] is not None else 6 * cus
    win_forced = sw["win_rows"] is not None
    p3l_max_rows = _nonneg(sw["p3l_rows"], 3 * cus)
    lpc_max = _nonneg(sw["lpc_max"], 64 * min(lpc_blocks, 3) * cus)
    dtc = ",true" if rep else ""
    w2ok = bool(flags & SERIES_WINDOW2_OK) or (bool(flags & SERIES_WINDOW2_SMALL) and B <= 2 * cus)
    if B <= win2_max_evals and win_max_rows > 0 and n >= 16 and (w2ok or win_forced):
        wgs = (B + 1) // 2
        sl = n <= W2_MAX_N
        pl.update(shape=WIN2, sl=sl, grid=wgs, block=256)
        if sl and wgs > cus:
            pl.update(ho=True, fold=p in (5, 7) and wgs <= 2 * cus)
        name = "k_logdens_carma_w2<%d>" % p
    elif rows <= win_max_rows and n >= 8 and ((flags & SERIES_WINDOW_OK) or win_forced):
        pl.update(shape=WIN, grid=rows, block=256)
        name = "k_logdens_carma_w<%d>" % p
    elif rows <= p3l_max_rows and n >= 8:
        pl.update(shape=P3L, grid=rows, block=256)
        name = "k_logdens_carma_p3l<%d>" % p
    elif B > lpc_min_evals(p, cus, sw) and B <= lpc_max and n >= 8:
        pl.update(shape=LPC, grid=(B + 63) // 64, block=256, unrolled=not rep and B <= 64 * cus,
                  rot=sw["lpc_rot"] if sw["lpc_rot"] is not None else 0x0202)
        name = "k_logdens_carma_lpc<%d,3%s>" % (p, dtc)
    elif B >= lane_min_evals(p, cus, sw):
        pl.update(shape=LANE, grid=(B + 63) // 64, block=64)
        name = "k_logdens_carma_lane<%d%s>" % (p, dtc)
    elif waves <= 256 and n >= 8:
        pl.update(shape=PC, pairs=1, grid=waves, block=128)
        name = "k_logdens_carma_pc<%d,%d,1>" % (p, G)
    elif waves <= 512 and n >= 8:
        pl.update(shape=PC, pairs=2, grid=(waves + 1) // 2, block=256)
        name = "k_logdens_carma_pc<%d,%d,2>" % (p, G)
    elif waves <= 2048:
        pl.update(shape=PLAIN, waves=1, grid=waves, block=64)
        name = "k_logdens_carma<%d,%d,1%s>" % (p, G, dtc)
    else:
        pl.update(shape=PLAIN, waves=4, grid=(waves + 3) // 4, block=256)
        name = "k_logdens_carma<%d,%d,4%s>" % (p, G, dtc)
    pl["name"] = name
    return pl


def logdens_car1(B, n, cus, sw=UNSET):
    smax = _nonneg(sw["car1_scan_max"], 48 * cus)
    scan = B <= smax and n >= 64
    return dict(shape=CAR1_SCAN if scan else CAR1_LANE, p=1, G=0, repeated_dt=False, sl=False, ho=False, fold=False, unrolled=False, pairs=0,
                waves=0, rot=0, grid=B if scan else (B + 63) // 64, block=64, name="k_logdens_car1")


def kernel_name(p, B, n, flags, cus, lpc_blocks=1, sw=UNSET):
    return logdens_car1(B, n, cus, sw)["name"] if p == 1 else logdens(p, B, n, flags, cus, lpc_blocks, sw)["name"]


LD_FIELDS = ("shape", "p", "G", "repeated_dt", "sl", "ho", "fold", "unrolled", "pairs", "waves", "rot", "grid", "block")


def ld_line(pl):
    return "ld " + " ".join(str(int(pl[k])) for k in LD_FIELDS) + " " + pl["name"]


# ---- sampler family (carma_pt_create) ------------------------------------------------------------------------------------------
def row_capacity(T, n, cus, row_per_cu, sw=UNSET):
    """row_per_cu: what the occupancy query gives for k_pt_row<P,3>; 0 where the row sampler does not apply"""
    if n < 32 or T < 1 or row_per_cu < 1:
        return 0
    per_cu = row_per_cu
    tune = sw["pt_row_wgs_per_cu"]
    if tune is not None and 0 < tune < per_cu:
        per_cu = tune
    return cus * min(per_cu, 3)


def family(p, T, R, n, cus, row_per_cu, force=None, lane_min=None, sw=UNSET):
    nchain = T * R
    lane = False
    if T <= 64:
        G = 2 if p == 2 else (4 if p <= 4 else 8)
        ladder_waves = R * ((T * G + 63) // 64)
        pays = ladder_waves > 4 * cus
        if p == 1:
            pays = n >= 64 and nchain >= 64 and not (nchain > 48 * cus and nchain <= 64 * cus)
        if p in (2, 3):
            pays = pays or nchain > 12 * cus
        if p in (4, 5):
            pays = pays or nchain > 16 * cus
        if lane_min is not None:
            pays = nchain >= lane_min
        lane = force == "lane" or (force is None and pays)
    if lane:
        return LANE_FAMILY
    if p >= 2 and force != "ladder" and row_capacity(T, n, cus, row_per_cu, sw) >= R * ((T + 3) // 4):
        return ROW
    return LADDER


# ---- row sampler (launch_pt_row_p) ---------------------------------------------------------------------------------------------
def row_lds(ring3l_bytes, T, n_series=0):
    """pt_row_lds: ring3l_bytes is Pipe3LGeom<2>::BYTES"""
    base = ring3l_bytes + (4 * PT_DMAX + 8 + 3 * T) * 8 + T * 8 + 16 + 128 * 8 + 16 + T * (PT_DMAX + 1) * 8
    if n_series > 0:
        return ((base + 15) & ~15) + 16 + (n_series + (n_series & 1)) * 24
    return base


def row(R, T, T_global, n, flags, cus, lds_global, sw=UNSET):
    ew = sw["pt_row_win"]
    grid2_global = R * ((T_global + 1) // 2)
    w2ok = bool(flags & SERIES_WINDOW2_OK) or (bool(flags & SERIES_WINDOW2_SMALL) and grid2_global <= cus)
    sl = n <= 1024 or (grid2_global <= cus and lds_global <= 160 * 1024)
    two = grid2_global <= 2 * cus and w2ok and n >= 32
    if ew is not None:
        two = ew == 2 and grid2_global <= 2 * cus and n >= 32
    wpl = (T + 1) // 2 if two else (T + 3) // 4
    grid = R * wpl
    minw = 3 if grid > 2 * cus else 2
    grid_global = R * ((T_global + 3) // 4)
    win = grid_global <= cus and bool(flags & SERIES_WINDOW_OK)
    if ew is not None:
        win = ew != 0 and minw < 3
    two = two and minw < 3
    win = win and minw < 3
    rot = 0x36D2 if wpl == 1 else 0xB14E
    if sw["pt_row_rot"] is not None and sw["pt_row_rot"] >= 0:
        rot = sw["pt_row_rot"]
    xcd = 8 if (wpl > 1 and R % 8 == 0) else 1
    tx = sw["pt_row_xcd_map"]
    if tx is not None and tx >= 0:
        xcd = tx if (tx > 1 and R % tx == 0) else 1
    return dict(two=two, win=win, minw=minw, ho=grid > cus, sl=sl, wpl=wpl, grid=grid, rot=rot, xcd_map=xcd, cooperative=wpl != 1,
                pipeline=2 if two else (1 if win else 0))


ROW_FIELDS = ("two", "win", "minw", "ho", "sl", "wpl", "grid", "rot", "xcd_map", "cooperative", "pipeline")
PIPELINES = ("one-datum", "window", "two-sided")


def row_instance(p, pl):
    """the instantiation of k_pt_row a plan launches, as pt_row_fn picked it"""
    if pl["two"] and not pl["sl"]:
        return "k_pt_row<%d,2,true,true,false,false>" % p
    if pl["two"]:
        return "k_pt_row<%d,2,true,true,%s>" % (p, "true" if pl["ho"] else "false")
    if pl["win"]:
        return "k_pt_row<%d,2,true>" % p
    return "k_pt_row<%d,%d>" % (p, pl["minw"])


# ---- ladder sampler (pt_lds_bytes, launch_pt_p) --------------------------------------------------------------------------------
def ladder(p, d, T, R, n, cus, ring_bytes, sw=UNSET):
    G = 4 if p <= 1 else group_of(p)
    nthr_c = ((T * G + 63) // 64) * 64
    per = 4 * d + d * d
    state = (T * per + 4 * T + T * d) * 8 + T * 8 + 16
    plain_lds = nthr_c * 48 + state
    with_ring = plain_lds + (nthr_c // 64) * ring_bytes
    fits = p >= 2 and 2 * nthr_c <= 1024 and with_ring <= 150 * 1024
    plain = R > cus
    if sw["pt_plain"] is not None and sw["pt_plain"] >= 0:
        plain = sw["pt_plain"] == 1
    pc = fits and n >= 32 and not plain
    nthr = 2 * nthr_c if pc else nthr_c
    return dict(fits_pc=fits, nthr_fit=2 * nthr_c if fits else nthr_c, lds_fit=with_ring if fits else plain_lds, pc=pc,
                maxt=256 if nthr <= 256 else 1024, nthr=nthr, lds=with_ring if pc else plain_lds)


LAD_FIELDS = ("fits_pc", "nthr_fit", "lds_fit", "pc", "maxt", "nthr", "lds")


def sw_words(sw):
    return " ".join("u" if sw[k] is None else str(int(sw[k])) for k in SW_NAMES)
