"""The planner of carma_bandset_smooth restated in numpy (carma_mband_set_smooth_plan.h), the stand-alone program that runs the
header (tests/mbandset_smooth/plan_main.cpp) and the random calls both are compared on -- test code only."""
import functools
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "carma_pack_amd", "csrc")
PLAN_SRC = os.path.join(HERE, "mbandset_smooth", "plan_main.cpp")
PLAN_EXE = os.path.join(HERE, "mbandset_smooth", "plan_main")
PLAN_SAN = os.path.join(HERE, "mbandset_smooth", "plan_main_san")
CAP = 256 << 20                                               # SMOOTH_SCRATCH_CAP


def nfields(p):
    return 2 * p + p // 2 + 5                                 # k, cr, sr of every pair, {pm, f, s, innov | slot, a}


def _build(exe, extra):
    srcs = [PLAN_SRC] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in srcs):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", CSRC] + extra + ["-o", exe, PLAN_SRC])
    return exe


@functools.lru_cache(None)
def plan_exe(sanitized=False):
    """The program; sanitized: built with -fsanitize=address,undefined (host code with its own main, run directly)."""
    if sanitized:
        return _build(PLAN_SAN, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    return _build(PLAN_EXE, [])


def _run(args, text, sanitized=False):
    r = subprocess.run([plan_exe(sanitized)] + [str(a) for a in args], input=text, capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    assert not sanitized or "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-2000:]
    return r.stdout


def _nums(a):
    return " ".join(repr(float(v)) for v in np.asarray(a, dtype=float).ravel())


def _ints(a):
    return " ".join(str(int(v)) for v in np.asarray(a).ravel())


def plan(p, nobj, t0, obj, band, times, toff0=0, forced=0, cap=0, sanitized=False):
    """mbandset_smooth_plan -> dict of its tables (row_idx as [W, 64], req as [., 4]); cap 0: the library's."""
    text = "%d\n%s\n%s\n%d %d\n" % (len(nobj), _ints(nobj), _nums(t0), len(obj), toff0)
    text += "".join("%d %d %d %s\n" % (obj[i], band[i], len(times[i]), _nums(times[i])) for i in range(len(obj)))
    out = _run(["plan", p, forced, cap], text, sanitized).split("\n")
    W, J, sc_max = (int(v) for v in out[0].split())
    names = ("wave_job", "job_obj", "job_band", "job_M", "job_req", "row_idx", "wave_sc", "out_off", "chunk0")
    pl = {k: np.array(out[1 + i].split(), dtype=np.int64) for i, k in enumerate(names)}
    pl.update(W=W, J=J, sc_max=sc_max, req=np.array(out[10].split(), dtype=float).reshape(-1, 4))
    pl["row_idx"] = pl["row_idx"].reshape(W, 64)
    return pl


def check(h=1, S=4, K=3, nobj=(6, 20, 40, 600), obj=(0, 3), band=(2, 0), toff=(5, 8, 9), tout=None, null=(), sanitized=False):
    """mbandset_smooth_check -> the message ("" = fine).  null: names of the pointers passed as NULL; tout: the whole array the
    offsets index (default: toff[-1] finite times)."""
    order = ("theta", "object", "band", "tout", "toff", "mean", "var")
    mask = sum(1 << order.index(n) for n in null)
    if tout is None:
        tout = 0.5 * np.arange(max(int(toff[-1]), 0))
    B = len(obj)
    text = "%d %d %d\n%s\n%d %d\n%s\n%s\n%s\n%d\n%s\n" % (h, S, K, _ints(nobj), B, mask, _ints(obj), _ints(band), _ints(toff),
                                                         len(tout), _nums(tout))
    return _run(["check"], text, sanitized).rstrip("\n")


def set_t0(objects):
    """(MbandSet::t0 [S], MbandObject::t0 of every object prepared alone [S])"""
    bands = [b for o in objects for b in o]
    off = np.concatenate([[0], np.cumsum([len(b[0]) for b in bands])])
    text = "%d %d\n%s\n" % (len(objects), len(objects[0]), _ints(off))
    text += "".join(_nums(np.concatenate([np.asarray(b[k], dtype=float) for b in bands])) + "\n" for k in range(3))
    out = _run(["t0"], text).split("\n")
    return np.array(out[0].split(), dtype=float), np.array(out[1].split(), dtype=float)


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def times_ref(tout, t0):
    """mband_smooth_times: the records [M + 1, 4] of one list of requested times."""
    tout = np.asarray(tout, dtype=float)
    perm = np.argsort(tout, kind="stable")
    rec = np.zeros((tout.size + 1, 4))
    rec[:-1, 0], rec[:-1, 1] = tout[perm] - t0, perm
    rec[-1] = [np.inf, 0.0, 1.0, 0.0]
    return rec


def plan_ref(p, nobj, t0, obj, band, times, forced=0, cap=CAP):
    """The plan from the description alone: jobs = runs of equal (object, band, number of times, times) in a stable sort, waves
    of 64 rows of a job in the caller's order, the waves by falling ng (stable), chunks cut at the cap or at `forced` waves."""
    B = len(obj)
    key = [(int(obj[i]), int(band[i]), len(times[i]), tuple(float(v) for v in times[i])) for i in range(B)]
    order = sorted(range(B), key=lambda i: key[i])
    jobs, waves = [], []                                      # waves: (job, rows)
    for i in order:
        if not jobs or key[jobs[-1][0]] != key[i]:
            jobs.append([])
        jobs[-1].append(i)
    req, job_req = [], []
    for j, rows in enumerate(jobs):
        job_req.append(sum(r.shape[0] for r in req))
        req.append(times_ref(times[rows[0]], t0[obj[rows[0]]]))
        waves += [(j, rows[a:a + 64]) for a in range(0, len(rows), 64)]
    ng = [int(nobj[obj[rows[0]]]) + len(times[rows[0]]) for rows in jobs]
    waves.sort(key=lambda w: -ng[w[0]])
    row_idx = np.full((len(waves), 64), -1, dtype=np.int64)
    for w, (_, rows) in enumerate(waves):
        row_idx[w, :len(rows)] = rows
    wave_sc, chunk0, used, nw, sc_max = [], [], 0, 0, 0
    for w, (j, _) in enumerate(waves):
        need = ng[j] * 64 * nfields(p)
        if w == 0 or (forced > 0 and nw >= forced) or 8 * (used + need) > cap:
            chunk0.append(w)
            used = nw = 0
        wave_sc.append(used)
        used += need
        nw += 1
        sc_max = max(sc_max, used)
    chunk0.append(len(waves))
    sizes = np.array([len(t) for t in times])
    return dict(W=len(waves), J=len(jobs), sc_max=sc_max, wave_job=np.array([w[0] for w in waves]),
                job_obj=np.array([obj[r[0]] for r in jobs]), job_band=np.array([band[r[0]] for r in jobs]),
                job_M=np.array([len(times[r[0]]) for r in jobs]), job_req=np.array(job_req), row_idx=row_idx,
                wave_sc=np.array(wave_sc), out_off=np.concatenate([[0], np.cumsum(sizes)[:-1]]), chunk0=np.array(chunk0),
                req=np.concatenate(req))


def random_call(seed, B, S=4, K=3):
    """A call of B rows on S objects: a pool of time lists of M = 1 ... 40 (unsorted, with repeats) that many rows share, so that
    equal lists meet on the same and on different objects and bands.  -> (nobj, t0, obj, band, times)"""
    rng = np.random.default_rng(seed)
    nobj = rng.integers(2, 700, S)
    t0 = np.round(rng.uniform(-50.0, 50.0, S), 2)
    pool = []
    for M in [1, 1, 2, 40, 40] + list(rng.integers(1, 41, 4)):
        t = 0.25 * rng.integers(-40, 400, M)
        if M > 2:
            t[-1] = t[0]                                      # a repeated time
        pool.append(t.astype(float))
    pool.append(pool[3][::-1].copy())                         # the same times in another order: another job
    few = rng.integers(0, S, 2), rng.integers(0, K, 2)        # two (object, band) pairs take most rows: jobs of several waves
    obj, band, times = [], [], []
    for i in range(B):
        k = int(rng.integers(0, 4)) // 2                      # (the first pair, on ONE list, takes half of them)
        busy = rng.uniform() < 0.75
        obj.append(int(few[0][k]) if busy else int(rng.integers(0, S)))
        band.append(int(few[1][k]) if busy else int(rng.integers(0, K)))
        mine = pool[3] if k == 0 else pool[(0, 3)[int(rng.integers(0, 2))]]
        times.append(mine if busy else pool[int(rng.integers(0, len(pool)))])
    return nobj, t0, obj, band, times
