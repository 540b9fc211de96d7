#!/usr/bin/env python3
"""One of the scan scripts (scan_bench.py, scan_headline.py, with its arguments) run unchanged in this process, then one
line `RESULT {json}`: the phases of its last scan (dcp_scan_last_timing), how that scan held its product rows
(dcp_scan_product_stats), the md5 of the products.tsv it wrote, what its product directory holds, and the process's
ru_maxrss -- one fresh process per measurement (profiles/r13_product_runs.txt)."""
import glob
import hashlib
import json
import os
import resource
import runpy
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if len(sys.argv) < 2:
    sys.exit("usage: scan_once.py scan_bench.py|scan_headline.py [its arguments]")
script = sys.argv[1]
sys.argv = [os.path.join(HERE, script)] + sys.argv[2:]
g = runpy.run_path(sys.argv[0], run_name="__main__")
scan = g["scan"]
t = scan.last_timing()
out = dict(script=script, total_s=t["total_s"], products_tsv_s=t["products_tsv_s"], rows_decode_s=t["rows_decode_s"],
           path_batches=t["path_batches"], product_stats=scan.product_stats(),
           budget_mb=os.environ.get("DECIPHON_HIP_PRODUCT_MB", "default"),
           maxrss_mb=resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1024.0)
last = sorted(glob.glob(os.path.join(g["tmp"], "prod*", "products.tsv")))[-1]
out["md5"] = hashlib.md5(open(last, "rb").read()).hexdigest()
out["product_dir"] = sorted(os.listdir(os.path.dirname(last)))
print("RESULT " + json.dumps(out), flush=True)
