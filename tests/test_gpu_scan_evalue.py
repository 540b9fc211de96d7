"""GPU: the evalue column of products.tsv and its row filter (dcp_scan_calibrate, dcp_scan_set_evalue), on
tests/golden/minifam.dcp with the consensus reads and again from minifam.hmm.  A scan that is not calibrated writes the
golden rows; a calibrated one changes column 11 alone, to the E-value host.lrt_evalue gives for the fp32 lrt an
Engine.cost of the row's window has; the filter leaves out exactly the rows at or beyond the limit."""
import math
import os

import numpy as np
import pytest

import deciphon_amd
from dcp_testlib import GOLDEN, bits, read_fasta
from deciphon_amd import host

pytestmark = pytest.mark.gpu

DCP = os.path.join(GOLDEN, "minifam.dcp")
HMM = os.path.join(GOLDEN, "minifam.hmm")
HEADER = ["sequence", "window", "window_start", "window_stop", "hit", "hit_start", "hit_stop", "profile", "abc", "lrt", "evalue",
          "match"]
CALIB = dict(nseq=64, length=120, seed=7, freq=None, lam=0.5)
LAMBDA = 0.5


def reads():
    return [(i, s) for i, (_, s) in enumerate(read_fasta(os.path.join(GOLDEN, "consensus.fna")))]


def make_scan(route, strands="plus", epsilon=0.01):
    from deciphon_amd.scan import Scan

    if route == "hmm":
        return Scan.from_hmm(HMM, 1, epsilon, strands=strands)
    return Scan(DCP, 0, 1, True, False, False, strands=strands)


def run(scan, out_dir):
    from deciphon_amd.scan import Batch, Sequence

    batch = Batch()
    for sid, text in reads():
        batch.add(Sequence(sid, f"seq{sid}", text))
    scan.run(str(out_dir), batch)
    rows = scan.products()
    lines = open(os.path.join(str(out_dir), "products.tsv")).read().splitlines()
    assert lines[0].split("\t")[:12] == HEADER
    assert lines[1:] == rows
    return [r.split("\t") for r in rows]


def golden_rows():
    return [ln.rstrip("\n").split("\t") for ln in open(os.path.join(GOLDEN, "products.tsv"))][1:]


def row_lrts(route, rows, strands, epsilon=0.01):
    """the fp32 lrt of every row's window from an Engine.cost, and the row's profile index"""
    with deciphon_amd.Engine(0) as eng:
        if route == "hmm":
            eng.load_hmm(HMM, 1, epsilon)
        else:
            eng.load_dcp(DCP)
        eng.commit()
        eng.set_mode(True, False)
        eng.set_sequences([deciphon_amd.encode(s) for _, s in reads()], strands=strands)
        index = {eng.accession(p): p for p in range(eng.num_profiles)}
        per = 2 if strands == "both" else 1
        wins, prof = [], []
        for r in rows:
            seq = int(r[0]) * per + (1 if per == 2 and r[12] == "-" else 0)
            prof.append(index[r[7]])
            wins.append((prof[-1], seq, int(r[2]), int(r[3])))
        nul, alt = eng.cost(np.array(wins, np.int32).reshape(-1, 4))
    return [host.lrt(-n, -a) for n, a in zip(nul, alt)], prof


def without_evalue(rows):
    return [r[:10] + r[11:] for r in rows]


@pytest.mark.parametrize("route", ["dcp", "hmm"])
def test_uncalibrated_rows_are_the_golden_rows(tmp_path, route):
    with make_scan(route) as scan:
        assert math.isnan(scan.profile_mu(0))
        scan.set_evalue(0.0, 0.0)  # no limit applies to a scan that is not calibrated
        rows = run(scan, tmp_path)
        assert math.isnan(scan.profile_mu(0))
    gold = golden_rows()
    assert len(rows) == len(gold) == 3
    for got, want in zip(rows, gold):
        assert got[:10] == want[:10] and got[10] == "nan" and got[11] == want[11]


@pytest.mark.parametrize("strands,z", [("plus", None), ("both", None), ("plus", 1000.0)])
@pytest.mark.parametrize("route", ["dcp", "hmm"])
def test_calibrated_rows_differ_in_the_evalue_alone(tmp_path, route, strands, z):
    with make_scan(route, strands) as scan:
        plain = run(scan, tmp_path / "plain")
        scan.calibrate(**CALIB)
        if z is not None:
            scan.set_evalue(z)
        rows = run(scan, tmp_path / "calibrated")
        mu = [scan.profile_mu(p) for p in range(3)]
    assert len(plain) >= 3 and all(r[10] == "nan" for r in plain)
    assert all(np.isfinite(mu))
    assert without_evalue(rows) == without_evalue(plain)
    lrts, prof = row_lrts(route, rows, strands)
    Z = z if z is not None else len(reads()) * (2 if strands == "both" else 1)
    for r, lrt, p in zip(rows, lrts, prof):
        assert "%.1f" % lrt == r[9]
        assert r[10] == "%.2g" % host.lrt_evalue(lrt, mu[p], LAMBDA, Z), (r[:11], lrt, mu[p], Z)


@pytest.mark.parametrize("route", ["dcp", "hmm"])
def test_filter(tmp_path, route):
    with make_scan(route) as scan:
        scan.calibrate(**CALIB)
        rows = run(scan, tmp_path / "all")
        mu = [scan.profile_mu(p) for p in range(3)]
        lrts, prof = row_lrts(route, rows, "plus")
        E = [host.lrt_evalue(lrt, mu[p], LAMBDA, len(reads())) for lrt, p in zip(lrts, prof)]
        assert len(set(E)) == len(E) == 3
        limit = float(np.median(E))
        scan.set_evalue(0.0, limit)
        kept = run(scan, tmp_path / "median")
        assert kept == [r for r, e in zip(rows, E) if e < limit] and len(kept) == 1
        scan.set_evalue(0.0, 1.0)  # the reference's rule: these are real domains
        assert run(scan, tmp_path / "one") == [r for r, e in zip(rows, E) if e < 1.0]
        scan.set_evalue(0.0, 0.0)
        assert run(scan, tmp_path / "none") == []
        assert open(os.path.join(str(tmp_path / "none"), "products.tsv")).read().splitlines() == ["\t".join(HEADER)]
        scan.set_evalue(0.0, float("inf"))
        assert run(scan, tmp_path / "again") == rows


def test_set_epsilon_makes_the_scan_uncalibrated(tmp_path):
    with make_scan("hmm") as scan:
        scan.calibrate(**CALIB)
        assert all(r[10] != "nan" for r in run(scan, tmp_path / "a"))
        scan.set_epsilon(0.02)
        assert all(math.isnan(scan.profile_mu(p)) for p in range(3))
        plain = run(scan, tmp_path / "b")
        assert len(plain) >= 1 and all(r[10] == "nan" for r in plain)
        scan.calibrate(**CALIB)
        mu = [bits(scan.profile_mu(p)) for p in range(3)]
        again = run(scan, tmp_path / "c")
        assert without_evalue(again) == without_evalue(plain) and all(r[10] != "nan" for r in again)
    with make_scan("hmm", epsilon=0.02) as fresh:
        fresh.calibrate(**CALIB)
        assert [bits(fresh.profile_mu(p)) for p in range(3)] == mu
        assert run(fresh, tmp_path / "d") == again


def test_calibrate_needs_a_setup_and_good_arguments():
    from deciphon_amd.scan import DeciphonError

    with make_scan("dcp") as scan:
        for kw in (dict(CALIB, lam=0.0), dict(CALIB, nseq=0), dict(CALIB, length=0), dict(CALIB, freq=[0, 0, 0, 0])):
            with pytest.raises(DeciphonError) as e:
                scan.calibrate(**kw)
            assert e.value.code == 8
        with pytest.raises(DeciphonError):
            scan.set_evalue(float("nan"), 1.0)
        assert math.isnan(scan.profile_mu(0)) and math.isnan(scan.profile_mu(99))
