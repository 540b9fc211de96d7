#!/usr/bin/env python3
"""Measures dcp_press on a Pfam-shaped synthetic HMMER3 file: lengths from synth.pfam_like_lengths, node values
resampled from tests/golden/minifam.hmm's three profiles (deciphon_amd.synth.pfam_like_hmms).  Prints seconds per
phase as dcp_press_last_timing reports them -- parse + model (host), upload, kernel and copy-back (GPU, HIP events),
host waiting for the GPU, write (records + header) -- nodes/s and output MB/s, and one JSON line."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from deciphon_amd import Press, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--profiles", type=int, default=1000)
ap.add_argument("--seed", type=int, default=1)
ap.add_argument("--epsilon", type=float, default=0.01)
ap.add_argument("--dir", default=None, help="where the .hmm and .dcp go (default: a temporary directory)")
ap.add_argument("--keep", action="store_true")
args = ap.parse_args()

work = args.dir or tempfile.mkdtemp(prefix="press_bench_")
os.makedirs(work, exist_ok=True)
hmm, dcp = os.path.join(work, "pfam_like.hmm"), os.path.join(work, "pfam_like.dcp")
seeds = synth.load_hmm_seeds(os.path.join(ROOT, "tests", "golden", "minifam.hmm"))
t0 = time.perf_counter()
synth.write_hmm(hmm, synth.pfam_like_hmms(seeds, args.profiles, args.seed))
t_gen = time.perf_counter() - t0

t0 = time.perf_counter()
with Press(hmm, dcp, 1, args.epsilon) as p:
    n = p.nproteins
    t_open = time.perf_counter() - t0
    while not p.end():
        p.next()
t_total = time.perf_counter() - t0
t = p.timing()  # close's header and copy of the records included
assert int(t["bytes"]) == os.path.getsize(dcp)
res = dict(profiles=n, nodes=int(t["nodes"]), hmm_mb=os.path.getsize(hmm) / 1e6, dcp_mb=t["bytes"] / 1e6,
           wall_s=t_total, open_s=t_open, parse_model_s=t["parse_model"], upload_s=t["upload"], kernel_s=t["kernel"],
           copy_back_s=t["copy_back"], gpu_wait_s=t["wait"], write_s=t["write"],
           nodes_per_s=t["nodes"] / t_total, out_mb_per_s=t["bytes"] / 1e6 / t_total,
           kernel_nodes_per_s=t["nodes"] / t["kernel"] if t["kernel"] else None, generate_s=t_gen)
for k in ("wall_s", "open_s", "parse_model_s", "upload_s", "kernel_s", "copy_back_s", "gpu_wait_s", "write_s"):
    print(f"{k:>14}: {res[k]:9.4f} s  ({100 * res[k] / t_total:5.1f} % of wall)")
print(f"{n} profiles, {res['nodes']} nodes, {res['dcp_mb']:.1f} MB out: {res['nodes_per_s']:.3g} nodes/s, "
      f"{res['out_mb_per_s']:.1f} MB/s")
print(json.dumps(res))
if not args.keep:
    for f in (hmm, dcp):
        os.unlink(f)
    if not args.dir:
        os.rmdir(work)
