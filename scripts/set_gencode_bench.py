#!/usr/bin/env python3
"""Resident profiles under another translation table, beside the reload it replaces, on the Pfam-shaped synthetic file
of press_bench.py and load_hmm_bench.py:

  (a) Engine.load_hmm at table 1, then Engine.set_gencode(11) on that engine: wall clock, and the seconds of host
      recomputation, upload and kernels that dcp_hip_set_gencode prints under DECIPHON_HIP_TIMING;
  (b) the yardstick, in the same process and build: a fresh Engine.load_hmm of the file at table 11, wall clock and the
      seconds of parsing dcp_hip_load_hmm prints;
  (c) the host recomputation alone (dcp_regencode_entries over every node of the file) on 1 and on 16 threads: what
      of the load's parsing seconds is the model building that set_gencode repeats, and how it spreads.

(a) and (b) alternate, --runs times each; (c) runs once per thread count after them.  Prints a line per measurement and
one JSON line; --out appends the printed lines to a file as well."""
import argparse
import json
import os
import re
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from deciphon_amd import Engine, host, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--profiles", type=int, default=2000)
ap.add_argument("--seed", type=int, default=1)
ap.add_argument("--epsilon", type=float, default=0.01)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--from-table", type=int, default=1)
ap.add_argument("--to-table", type=int, default=11)
ap.add_argument("--dir", default=None, help="where the .hmm goes (default: a temporary directory)")
ap.add_argument("--out", default=None, help="a file the printed lines are appended to")
args = ap.parse_args()

work = args.dir or tempfile.mkdtemp(prefix="set_gencode_bench_")
os.makedirs(work, exist_ok=True)
hmm = os.path.join(work, "pfam_like.hmm")
seeds = synth.load_hmm_seeds(os.path.join(ROOT, "tests", "golden", "minifam.hmm"))
nprof = synth.write_hmm(hmm, synth.pfam_like_hmms(seeds, args.profiles, args.seed))

LOAD = re.compile(r"dcp_hip_load_hmm: (\d+) profiles, ([\d.]+) GB of tables; parse ([\d.]+) s, upload ([\d.]+) s, "
                  r"emission kernel ([\d.]+) s, rows kernel ([\d.]+) s, wait ([\d.]+) s")
SET = re.compile(r"dcp_hip_set_gencode: (\d+) profiles, (\d+) nodes, table (\d+), (\d+) error rates; host recomputation "
                 r"([\d.]+) s, upload ([\d.]+) s, kernels ([\d.]+) s, wall ([\d.]+) s")


def say(line):
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


def stderr_of(call):
    """Runs call() with the process's stderr (the library writes to it) going to a file; -> (result, text)."""
    sys.stderr.flush()
    keep = os.dup(2)
    with tempfile.TemporaryFile() as f:
        os.dup2(f.fileno(), 2)
        try:
            out = call()
        finally:
            os.dup2(keep, 2)
            os.close(keep)
        f.seek(0)
        return out, f.read().decode(errors="replace")


def timed_load(eng, table):
    t0 = time.perf_counter()
    _, text = stderr_of(lambda: eng.load_hmm(hmm, table, args.epsilon))
    wall = time.perf_counter() - t0
    m = LOAD.search(text)
    assert m, text
    return wall, float(m.group(3))


def set_gencode_leg():
    with Engine(0) as eng:
        load_s, parse_s = timed_load(eng, args.from_table)
        t0 = time.perf_counter()
        _, text = stderr_of(lambda: eng.set_gencode(args.to_table))
        wall = time.perf_counter() - t0
        m = SET.search(text)
        assert m, text
        assert eng.profile_gencode(0) == args.to_table
        g = m.groups()
        return dict(first_load_s=load_s, first_parse_s=parse_s, set_gencode_s=wall, profiles=int(g[0]), nodes=int(g[1]),
                    host_s=float(g[4]), upload_s=float(g[5]), kernels_s=float(g[6]), pool_bytes=eng.pool_bytes,
                    dist_bytes=eng.dist_bytes)


def reload_leg():
    with Engine(0) as eng:
        load_s, parse_s = timed_load(eng, args.to_table)
        return dict(load_s=load_s, parse_s=parse_s)


os.environ["DECIPHON_HIP_TIMING"] = "1"
res = dict(profiles=nprof, hmm_mb=os.path.getsize(hmm) / 1e6, epsilon=args.epsilon, tables=[args.from_table, args.to_table],
           set_gencode=[], reload=[], host_recomputation={})
say(f"set_gencode_bench: {nprof} profiles, {res['hmm_mb']:.1f} MB of HMMER3 text, epsilon {args.epsilon}, table "
    f"{args.from_table} -> {args.to_table}, {os.cpu_count()} CPUs seen")
for run in range(args.runs):
    r = set_gencode_leg()
    res["set_gencode"].append(r)
    say(f"run {run} (a) set_gencode: {r['set_gencode_s']:.4f} s wall; host recomputation {r['host_s']:.4f}, upload "
        f"{r['upload_s']:.4f}, kernels {r['kernels_s']:.4f} s; {r['profiles']} profiles, {r['nodes']} nodes, pool "
        f"{r['pool_bytes'] / 1e9:.2f} GB (the load before it: {r['first_load_s']:.3f} s, parse {r['first_parse_s']:.3f})")
    r = reload_leg()
    res["reload"].append(r)
    say(f"run {run} (b) fresh load_hmm at table {args.to_table}: {r['load_s']:.3f} s wall, parse {r['parse_s']:.3f} s")
del os.environ["DECIPHON_HIP_TIMING"]

with host.HmmFile(hmm, args.from_table) as h:
    lodds = np.concatenate([p["lodds"] for p in h])
for threads in (1, 16):
    best = None
    for _ in range(2):
        t0 = time.perf_counter()
        host.regencode_entries(args.to_table, lodds, threads)
        t = time.perf_counter() - t0
        best = t if best is None else min(best, t)
    res["host_recomputation"][threads] = best
    say(f"(c) dcp_regencode_entries of {len(lodds)} nodes on {threads:2d} thread{'s' if threads > 1 else ' '}: {best:.4f} s "
        f"({best / len(lodds) * 1e6:.2f} us per node), the better of two")
a = sorted(r["set_gencode_s"] for r in res["set_gencode"])
b = sorted(r["load_s"] for r in res["reload"])
if a and b:
    say(f"set_gencode {a[0]:.4f} .. {a[-1]:.4f} s against the reload's {b[0]:.3f} .. {b[-1]:.3f} s over {args.runs} runs: "
        f"{b[len(b) // 2] / a[len(a) // 2]:.1f} x by the medians")
print(json.dumps(res))
os.unlink(hmm)
if not args.dir:
    os.rmdir(work)
