#!/usr/bin/env python3
"""Both strands in one dcp_scan_run against what a caller did before: on scan_headline.py's workload, in one process
and on one resident database, alternated --
  (a) one run with strands = both;
  (b) a plain run of the reads and a plain run of their host-made reverse complements;
  (c) a plain run alone.
Seconds per scan, the phases of dcp_scan_last_timing, the rows, and whether the rows of (a) are those of (b) with the
strand column added, in (profile, read, strand, window) order."""
import argparse
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench
from deciphon_amd import synth
from deciphon_amd.scan import Batch, Scan, Sequence

ap = argparse.ArgumentParser()
ap.add_argument("--profiles", type=int, default=400)
ap.add_argument("--reads", type=int, default=500)
ap.add_argument("--read-len", type=int, default=10000)
ap.add_argument("--repeat", type=int, default=3, help="timed rounds of (a), (b), (c), after one untimed round")
ap.add_argument("--out", help="also write the report here")
args = ap.parse_args()

lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


seeds = synth.load_seeds(bench.SEED_DB)
Ks = synth.pfam_like_lengths(args.profiles, bench.SEED)
prots = synth.pfam_like_database(seeds, args.profiles, bench.SEED, lengths=Ks)
tmp = tempfile.mkdtemp()
dcp = os.path.join(tmp, "pfam_like.dcp")
synth.write_dcp(dcp, prots, 0.01, False, False)
stride = max(1, len(Ks) // 48)
cons = [prots[i]["consensus"] for i in range(0, len(Ks), stride)]
reads = synth.synth_reads(args.reads, args.read_len, cons, bench.SEED)
texts = ["".join("ACGT"[v] for v in r) for r in reads]
t0 = time.perf_counter()
rc_texts = [t[::-1].translate(str.maketrans("ACGT", "TGCA")) for t in texts]
t_rc = time.perf_counter() - t0


def batch_of(ts):
    b = Batch()
    for i, t in enumerate(ts):
        b.add(Sequence(i, f"read{i}", t))
    return b


given, reversed_ = batch_of(texts), batch_of(rc_texts)
scan = Scan(dcp, 0, 1, True, False, False)
order = {p["accession"]: i for i, p in enumerate(prots)}
PHASES = ("reads_h2d_encode_s", "window_bookkeeping_s", "cost_pass_s", "path_pass_s", "rows_decode_s", "products_tsv_s")
runs = {"a": [], "b": [], "c": []}
n = 0


def one(strands, batch):
    global n
    n += 1
    scan.set_strands(strands)
    t = time.perf_counter()
    scan.run(os.path.join(tmp, f"prod{n}"), batch)  # (returns with products.tsv written: the GPU is idle again)
    dt = time.perf_counter() - t
    return dt, scan.last_timing(), scan.products()


def add(x, y):
    return {k: x[k] + y[k] for k in x}


say(f"strands_bench: {args.profiles} profiles (sum K {int(Ks.sum())}), {args.reads} reads of {args.read_len} nt; "
    f"reverse complements made on the host in {t_rc * 1e3:.1f} ms (not in any figure below)")
same = None
for rep in range(args.repeat + 1):
    ta, pa, ra = one("both", given)
    tp, pp, rp = one("plus", given)
    tm, pm, rm = one("plus", reversed_)
    tc, pc, rcw = one("plus", given)
    if rep == 0:  # the untimed round also compares the rows
        def key(r):
            f = r.split("\t")
            return order[f[7]], int(f[0]), f[12] == "-", int(f[1])

        merged = sorted([r + "\t+" for r in rp] + [r + "\t-" for r in rm], key=key)
        same = merged == ra
        say(f"rows: (a) {len(ra)} = {sum(r.endswith(chr(9) + '+') for r in ra)} plus + "
            f"{sum(r.endswith(chr(9) + '-') for r in ra)} minus; (b) {len(rp)} + {len(rm)}; (c) {len(rcw)}; "
            f"rows of (a) == rows of (b) with the strand column, merged: {same}")
        continue
    runs["a"].append((ta, pa))
    runs["b"].append((tp + tm, add(pp, pm)))
    runs["c"].append((tc, pc))
    say(f"round {rep}: (a) {ta:.3f} s   (b) {tp:.3f} + {tm:.3f} = {tp + tm:.3f} s   (c) {tc:.3f} s")

say()
say(f"{'':28s}{'(a) both, one run':>20s}{'(b) two plain runs':>20s}{'(c) one plain run':>20s}")
med = lambda xs: statistics.median(xs)
say(f"{'seconds per scan (median)':28s}" + "".join(f"{med([t for t, _ in runs[k]]):20.3f}" for k in "abc"))
say(f"{'seconds per scan (min..max)':28s}" + "".join(
    f"{min(t for t, _ in runs[k]):12.3f}..{max(t for t, _ in runs[k]):.3f}" for k in "abc"))
for ph in PHASES + ("windows", "path_passes", "rounds", "chunks"):
    fmt = "20.4f" if ph.endswith("_s") else "20.0f"
    say(f"{ph:28s}" + "".join(format(med([p[ph] for _, p in runs[k]]), fmt) for k in "abc"))
# the upload + encode phase is a host-timed interval of a millisecond or two: its spread over the rounds beside its median
h2d = {k: [p["reads_h2d_encode_s"] * 1e3 for _, p in runs[k]] for k in "abc"}
say(f"{'reads_h2d_encode ms min/med/max':32s}" + "".join(f"{min(h2d[k]):8.3f}/{med(h2d[k]):.3f}/{max(h2d[k]):.3f}" for k in "abc"))
a, b, c = (med([t for t, _ in runs[k]]) for k in "abc")
say()
say(f"(a) / (c) = {a / c:.2f}, (a) / (b) = {a / b:.2f}; cost pass (a) / (c) = "
    f"{med([p['cost_pass_s'] for _, p in runs['a']]) / med([p['cost_pass_s'] for _, p in runs['c']]):.2f}")
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
sys.exit(0 if same else 1)
