#!/usr/bin/env python3
"""A scan over all the GPUs of a node: torchrun --nproc-per-node N scripts/scan_multi_gpu.py db.dcp reads.fna outdir
(one process per GPU, contiguous profile partitions, rows gathered in partition order on rank 0).  The options are
what a single-GPU scan takes (deciphon_amd.dist.scan_partitioned)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deciphon_amd import dist

ap = argparse.ArgumentParser(description=__doc__)
ap.add_argument("dbfile")
ap.add_argument("fasta")
ap.add_argument("outdir")
ap.add_argument("--strands", choices=("plus", "both"), default="plus")
ap.add_argument("--calibrate", help="L1,L2,...: calibrate every profile over this ladder of read lengths")
ap.add_argument("--nseq", type=int, default=200, help="random reads per length of --calibrate")
ap.add_argument("--lam", type=float, default=0.5, help="lambda of --calibrate; 0 fits one per profile")
ap.add_argument("--evalue-max", type=float, default=float("inf"))
args = ap.parse_args()
seqs, name, chunks = [], None, []
for line in open(args.fasta):
    line = line.strip()
    if line.startswith(">"):
        if name is not None:
            seqs.append((len(seqs), name, "".join(chunks)))
        name, chunks = line[1:].split()[0], []
    elif line:
        chunks.append(line)
if name is not None:
    seqs.append((len(seqs), name, "".join(chunks)))
os.makedirs(args.outdir, exist_ok=True)
calibrate = None
if args.calibrate:
    calibrate = dict(nseq=args.nseq, lengths=tuple(int(v) for v in args.calibrate.split(",")), lam=args.lam)
rows = dist.scan_partitioned(args.dbfile, seqs, args.outdir, strands=args.strands, calibrate=calibrate,
                             evalue_max=args.evalue_max)
rank, _, world = dist.env_rank()
if rank == 0:
    print(f"{len(rows)} product rows from {world} partition(s) -> {os.path.join(args.outdir, 'products.tsv')}")
