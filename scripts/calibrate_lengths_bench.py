#!/usr/bin/env python3
"""Calibration over a ladder of read lengths, measured: the Pfam-shaped profile set of scripts/calibrate_bench.py, a
ladder of 300, 1000, 3000 and 10000 nt x 200 random reads, and what three calibrations say about a SECOND set of random
reads from other seeds, at the rung lengths and between them (550, 1800, 5500 nt):

    (a) one length, 300 nt, lambda = 0.5      Engine.calibrate
    (b) the ladder, lambda = 0.5              Engine.calibrate_lengths
    (c) the ladder, lambda fitted per profile Engine.calibrate_lengths(lam=0)

If lrt of a random read followed the Gumbel distribution (mu of its profile at the read's length, lambda of its profile),
P <= 0.05 would hold for 5 % of the second set and P <= 0.01 for 1 %.

    python scripts/calibrate_lengths_bench.py [--profiles 400] [--nseq 200] [--ladder 300,1000,3000,10000]
                                              [--between 550,1800,5500]

Prints the two shares per length under each calibration, the spread of the fitted lambda, and the seconds of each
call.  One MI355X run is kept in profiles/calibrate_lengths.txt."""
import argparse
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scripts.calibrate_bench import SEED, SEED_DB, lrt_of, windows  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--profiles", type=int, default=400)
    ap.add_argument("--nseq", type=int, default=200)
    ap.add_argument("--ladder", default="300,1000,3000,10000")
    ap.add_argument("--between", default="550,1800,5500")
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    ladder = [int(v) for v in args.ladder.split(",")]
    lengths = sorted(set(ladder) | {int(v) for v in args.between.split(",") if v})

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
            second = args.seed + 1000  # rung j of the ladder uses seed + j: the second set stays clear of them
            print(f"{n} Pfam-shaped profiles (sum K = {int(Ks.sum())}), ladder {ladder} x {args.nseq} uniform random reads, seed "
                  f"{args.seed}; second set: {args.nseq} reads per length from seeds {second}..")
            eng.calibrate(8, 60, args.seed)  # warm-up: streams, buffers, the special-transition table

            def timed(call):
                t0 = time.perf_counter()
                call()
                return time.perf_counter() - t0

            def rungs():
                lens = eng.calib_lengths
                mu = np.array([[eng.profile_mu_rung(p, j) for j in range(len(lens))] for p in range(n)], np.float32)
                lam = np.array([eng.profile_lambda(p) for p in range(n)], np.float64)
                excluded = sum(eng.profile_calib_excluded_rung(p, j) for p in range(n) for j in range(len(lens)))
                return lens, mu, lam, excluded

            fits = {}
            s = timed(lambda: eng.calibrate(args.nseq, ladder[0], args.seed, None, 0.5))
            fits[f"(a) {ladder[0]} nt, lambda 0.5"] = (s, rungs())
            s = timed(lambda: eng.calibrate_lengths(args.nseq, ladder, args.seed, None, 0.5))
            fits["(b) ladder, lambda 0.5"] = (s, rungs())
            s = timed(lambda: eng.calibrate_lengths(args.nseq, ladder, args.seed, None, 0.0))
            fits["(c) ladder, lambda fitted"] = (s, rungs())
            cells = float(Ks.sum()) * args.nseq
            for name, (s, (lens, mu, lam, excluded)) in fits.items():
                c = cells * sum(lens)
                print(f"{name}: {s:.3f} s for {c:.3g} cells ({c / s / 1e12:.2f} TCUPS), {excluded} scores excluded, "
                      f"{int(np.isnan(lam).sum())} profiles without a fit")
            lens, mu, lam, _ = fits["(c) ladder, lambda fitted"][1]
            print(f"fitted lambda over the profiles: min {np.nanmin(lam):.3f}, 5 % {np.nanpercentile(lam, 5):.3f}, median "
                  f"{np.nanmedian(lam):.3f}, 95 % {np.nanpercentile(lam, 95):.3f}, max {np.nanmax(lam):.3f}, sd {np.nanstd(lam):.3f}")
            for j, length in enumerate(lens):
                print(f"    mu at {length:6d} nt: (b) median {np.median(fits['(b) ladder, lambda 0.5'][1][1][:, j]):.2f}, (c) median "
                      f"{np.nanmedian(mu[:, j]):.2f}")

            # the second set, scored once per length
            total = {name: [0, 0, 0] for name in fits}
            print("share of the second set called at P <= 0.05 | P <= 0.01 (a random read should be, 5 % | 1 % of the time):")
            print(f"{'length':>8}  " + "  ".join(f"{name:>28}" for name in fits))
            for k, length in enumerate(lengths):
                eng.set_random_sequences(args.nseq, length, second + k)
                nul, alt = eng.cost(windows(n, args.nseq, length))
                x = lrt_of(nul, alt).reshape(n, args.nseq).astype(np.float64)
                ok = np.isfinite(x)
                cols = []
                for name, (_, (lens, mu, lam, _)) in fits.items():
                    at = np.array([host.calib_mu_at(lens, mu[p], length) for p in range(n)])
                    with np.errstate(invalid="ignore"):
                        P = -np.expm1(-np.exp(-lam[:, None] * (x - at[:, None])))
                    use = ok & np.isfinite(P)
                    total[name][0] += int((P[use] <= 0.05).sum())
                    total[name][1] += int((P[use] <= 0.01).sum())
                    total[name][2] += int(use.sum())
                    cols.append(f"{100 * (P[use] <= 0.05).mean():12.2f} % | {100 * (P[use] <= 0.01).mean():6.2f} %")
                mark = " " if length in ladder else "*"
                print(f"{length:7d}{mark}  " + "  ".join(f"{c:>28}" for c in cols), flush=True)
            print(f"{'all':>8}  " + "  ".join(f"{100 * a / m:12.2f} % | {100 * b / m:6.2f} %".rjust(28) for a, b, m in total.values()))
            print("(* between the rungs)")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
