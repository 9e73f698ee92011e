#!/usr/bin/env python3
"""Markdown table of the largest fraction of each allowance that tests/test_gpu_chaindiag.py consumed, from the
"chaindiag-allowance ..." lines of a `pytest -s` run of it:

    python -m pytest tests/test_gpu_chaindiag.py -m gpu -s -q > run.log;  python tools/chaindiag_allowance.py run.log"""
import re
import sys

worst, rows = {}, []
for line in open(sys.argv[1]):
    m = re.search(r"chaindiag-allowance (.*?) (L=\d+ d=\d+ R=\d+ G=\d+) levels<=(\d+) ok=(\d+) short=(\d+) :: (.*)", line)
    if not m:
        continue
    fr = dict((k, float(v)) for k, v in (kv.split("=") for kv in m.group(6).split()))
    rows.append((m.group(1), m.group(2), m.group(3), m.group(4), m.group(5), fr))
    for k, v in fr.items():
        worst[k] = max(worst.get(k, 0.0), v)
print("| case | shape | levels | OK | SHORT | mean | tau | sigma^2 | rhat |")
print("|---|---|---|---|---|---|---|---|---|")
for tag, shape, lev, ok, sh, fr in rows:
    print("| %s | %s | %s | %s | %s | %s |" % (tag, shape, lev, ok, sh, " | ".join("%.2g" % fr[k] if k in fr else "–" for k in ("mean", "tau", "sigma2", "rhat"))))
print("\nlargest fraction of an allowance used: " + ", ".join("%s %.2g" % kv for kv in sorted(worst.items())))
