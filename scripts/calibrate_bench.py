#!/usr/bin/env python3
"""Calibration on the GPU, measured: dcp_hip_calibrate over the benchmark's Pfam-shaped profile set at read lengths 300,
3000 and 10000, against the host route (numpy reads -> set_sequences -> cost -> numpy fit), and what the fitted
distribution says about a SECOND set of random reads from another seed: if lrt of a random read followed the Gumbel
distribution (mu of its profile, lambda), P <= 0.05 would hold for 5 % of them and P <= 0.01 for 1 %.

    python scripts/calibrate_bench.py [--profiles 400] [--nseq 200] [--lengths 300,3000,10000] [--lam 0.5]

Prints per length the spread of mu over the profiles, the two shares, and the seconds of either route.  One MI355X run
is kept in profiles/calibrate.txt."""
import argparse
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 20250310  # bench.py's
SEED_DB = os.path.join(ROOT, "tests", "golden", "minifam.dcp")


def windows(nprof, nseq, length):
    w = np.empty((nprof, nseq, 4), np.int32)
    w[:, :, 0] = np.arange(nprof, dtype=np.int32)[:, None]
    w[:, :, 1] = np.arange(nseq, dtype=np.int32)[None]
    w[:, :, 2] = 0
    w[:, :, 3] = length
    return w.reshape(-1, 4)


def lrt_of(nul, alt):
    return (np.float32(-2.0) * ((-nul) - (-alt))).astype(np.float32)


def fit(x, lam):
    """mu per row of x[nprof][nseq], as the kernel fits it, in float64"""
    x = x.astype(np.float64)
    m = x.min(axis=1, keepdims=True)
    return (m[:, 0] - np.log(np.exp(-lam * (x - m)).mean(axis=1)) / lam)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--profiles", type=int, default=400)
    ap.add_argument("--nseq", type=int, default=200)
    ap.add_argument("--lengths", default="300,3000,10000")
    ap.add_argument("--lam", type=float, default=0.5)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()

    import deciphon_amd
    from deciphon_amd import host, synth

    tmp = tempfile.mkdtemp(prefix="dcp_calib_")
    try:
        seeds = synth.load_seeds(SEED_DB)
        Ks = synth.pfam_like_lengths(args.profiles, SEED)
        dcp = os.path.join(tmp, "pfam_like.dcp")
        synth.write_dcp(dcp, synth.iter_pfam_like(seeds, len(Ks), SEED, lengths=Ks), 0.01, False, False)
        with deciphon_amd.Engine(0) as eng:
            eng.load_dcp(dcp)
            eng.commit()
            eng.set_mode(True, False)
            n = eng.num_profiles
            print(f"{n} Pfam-shaped profiles (sum K = {int(Ks.sum())}), {args.nseq} uniform random reads per length, "
                  f"lambda = {args.lam}, seeds {args.seed} (calibration) and {args.seed + 1} (second set)")
            eng.calibrate(8, 60, args.seed, None, args.lam)  # warm-up: streams, buffers, the special-transition table
            for length in [int(v) for v in args.lengths.split(",")]:
                w = windows(n, args.nseq, length)
                cells = float(Ks.sum()) * args.nseq * length
                t0 = time.perf_counter()
                eng.calibrate(args.nseq, length, args.seed, None, args.lam)
                gpu_s = time.perf_counter() - t0
                mu = np.array([eng.profile_mu(p) for p in range(n)], np.float64)
                excluded = sum(eng.profile_calib_excluded(p) for p in range(n))
                # the host route: the same reads made by numpy, uploaded, scored, fitted on the host
                t0 = time.perf_counter()
                nt = host.random_nt(args.seed, args.nseq * length)
                eng.set_sequences([nt[s * length:(s + 1) * length] for s in range(args.nseq)])
                nul, alt = eng.cost(w)
                mu_host = fit(lrt_of(nul, alt).reshape(n, args.nseq), args.lam)
                host_s = time.perf_counter() - t0
                # a second set of random reads, scored against the fit of the first
                eng.set_random_sequences(args.nseq, length, args.seed + 1)
                nul, alt = eng.cost(w)
                x = lrt_of(nul, alt).reshape(n, args.nseq).astype(np.float64)
                ok = np.isfinite(x)
                P = -np.expm1(-np.exp(-args.lam * (x - mu[:, None])))
                print(f"len {length:6d}: {cells:.3g} cells; GPU calibrate {gpu_s:.3f} s ({cells / gpu_s / 1e12:.2f} TCUPS), host route "
                      f"{host_s:.3f} s; mu min {mu.min():.2f} median {np.median(mu):.2f} max {mu.max():.2f} sd {mu.std():.2f}, "
                      f"excluded {excluded}, max |mu - host fit| {np.abs(mu - mu_host).max():.2e}; second set: "
                      f"P <= 0.05 for {100 * (P[ok] <= 0.05).mean():.2f} %, P <= 0.01 for {100 * (P[ok] <= 0.01).mean():.2f} % "
                      f"of {int(ok.sum())} scores", flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
