#!/usr/bin/env python3
"""Times carma_chain_diag -- the whole call (copies included) and its kernels alone (carma_chain_diag_kernel_ms) -- at the two
sizes of a set run, against (a) the numpy restatement tests/chaindiag_ref.py on the host for the same array and (b) the time to
read the input twice from HBM at 6.3 TB/s (the achievable rate; 8 TB/s is the data-sheet peak).  Well-mixed (phi = 0.3) and slow
(phi = 0.97) AR(1) chains separately: the halving makes their costs differ.

    python tools/chaindiag_probe.py [--reps 3] [--ref-groups N] [--small]

--ref-groups N: time the restatement on the first N groups only and scale (default: the whole array).  One JSON line per run."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import chaindiag_ref as cr  # noqa: E402
from carma_pack_amd import _lib  # noqa: E402

HBM = 6.3e12

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--ref-groups", type=int, default=0)
ap.add_argument("--small", action="store_true", help="a hundredth of the groups (a dry run of the tool)")
args = ap.parse_args()

SIZES = [(1024, 1, 20000, 11), (64, 4, 50000, 11)]
for S, R, L, d in SIZES:
    if args.small:
        S = max(1, S // 100)
    for phi in (0.3, 0.97):
        x = cr.ar1_block(1, S, R, L, [phi] * d, [0.0, 1.0, -3.0, 10.0, 100.0, 0.0, 1.0, -3.0, 10.0, 100.0, 0.0][:d])
        _lib.chain_diag(x[:1])                                         # first touch of the device
        call, kern = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            got = _lib.chain_diag(x)
            call.append(time.perf_counter() - t0)
            kern.append(_lib.chain_diag_kernel_ms() * 1e-3)
        ng = S if args.ref_groups <= 0 else min(S, args.ref_groups)
        t0 = time.perf_counter()
        ref = cr.chain_diag(x[:ng])
        t_ref = (time.perf_counter() - t0) * S / ng
        same = bool(np.array_equal(ref["status"], got["status"][:ng]))
        with np.errstate(all="ignore"):
            ok = np.isfinite(ref["tau"])
            dev = float(np.max(np.abs(got["tau"][:ng][ok] / ref["tau"][ok] - 1.0), initial=0.0))
        two_reads = 2.0 * x.nbytes / HBM
        print(json.dumps(dict(S=S, R=R, L=L, d=d, phi=phi, gbytes=round(x.nbytes / 1e9, 3), levels_max=int(ref["nlevels"].max()),
                              call_s=round(min(call), 4), kernel_s=round(min(kern), 5), numpy_s=round(t_ref, 2), numpy_groups=ng,
                              two_reads_s=round(two_reads, 6), numpy_over_call=round(t_ref / min(call), 1),
                              numpy_over_kernel=round(t_ref / min(kern), 1), kernel_over_two_reads=round(min(kern) / two_reads, 2),
                              status_equal=same, tau_max_rel_dev=dev)), flush=True)
        del x, got, ref
