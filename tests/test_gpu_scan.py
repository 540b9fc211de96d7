"""GPU: the reference's outer API (dcp_scan_* / dcp_batch_*, include/deciphon.h) through the
Python mirror of python-core's Scan/Batch classes -- the shape of python-core/tests/test_scan.py
and c-core/test_scan.c, test_window.c.  Expected rows come from the reference's committed
products.tsv (every column but the HMMER e-value, which is out of scope) and from an oracle-driven
restatement of thread_run."""
import os

import numpy as np
import pytest

import dcp_testlib
from dcp_testlib import GOLDEN, read_fasta
from oracle.dcp_reader import read_dcp

pytestmark = pytest.mark.gpu

DCP = os.path.join(GOLDEN, "minifam.dcp")


def oracle_scan(orc, db, reads, multi_hits, hmmer3_compat):
    return dcp_testlib.oracle_scan(orc, db.proteins, reads, multi_hits, hmmer3_compat)


def run_scan(tmp_path, reads, multi_hits=True, hmmer3_compat=False, dbfile=DCP, **kw):
    from deciphon_amd.scan import Batch, Scan, Sequence

    batch = Batch()
    for sid, text in reads:
        batch.add(Sequence(sid, f"seq{sid}", text))
    with Scan(dbfile, 0, 1, multi_hits, hmmer3_compat, False, **kw) as scan:
        scan.run(tmp_path, batch)
        assert scan.progress() == 100
        rows = scan.products()
    lines = open(os.path.join(tmp_path, "products.tsv")).read().splitlines()
    assert lines[0].split("\t") == ["sequence", "window", "window_start", "window_stop", "hit", "hit_start",
                                    "hit_stop", "profile", "abc", "lrt", "evalue", "match"]
    assert lines[1:] == rows
    return rows


def test_consensus_scan_matches_reference_products(tmp_path, orc):
    """control/tests/files/consensus.fna x minifam.dcp == control/tests/files/snap.dcs."""
    reads = [(i, s) for i, (_, s) in enumerate(read_fasta(os.path.join(GOLDEN, "consensus.fna")))]
    rows = run_scan(str(tmp_path), reads)
    gold = [ln.rstrip("\n").split("\t") for ln in open(os.path.join(GOLDEN, "products.tsv"))][1:]
    assert len(rows) == len(gold) == 3
    for got, want in zip(rows, gold):
        g = got.split("\t")
        assert g[:10] == want[:10]  # sequence .. lrt, byte for byte
        assert g[10] == "nan"       # evalue: HMMER (h3daemon) is out of scope
        assert g[11] == want[11]    # match: nucleotides, state, codon and amino of every step, byte for byte


@pytest.mark.parametrize("multi_hits,hmmer3_compat", [(True, False), (False, False), (True, True), (False, True)])
def test_all_reads_all_modes_against_oracle_scan(tmp_path, orc, multi_hits, hmmer3_compat):
    """The 8 reads of c-core/test_consensus.h x the 4 mode combinations of c-core/test_scan.c:15-16."""
    named = read_fasta(os.path.join(GOLDEN, "consensus.fna")) + read_fasta(os.path.join(GOLDEN, "consensus_multi.fna"))
    reads = [(i + 1, s) for i, (_, s) in enumerate(named)]
    rows = run_scan(str(tmp_path), reads, multi_hits, hmmer3_compat)
    assert rows == oracle_scan(orc, read_dcp(DCP), reads, multi_hits, hmmer3_compat)
    assert len(rows) >= 8


def test_sliding_windows_chain_like_test_window(tmp_path, orc):
    """c-core/test_window.c:25-37: a long read made of consensus copies with 70 % of the
    positions randomised, scanned through chained windows (window = 50*K nt)."""
    rng = np.random.default_rng(31)
    cons = read_fasta(os.path.join(GOLDEN, "consensus.fna"))[0][1]
    text = list((cons * 40)[:20000])
    for i in range(len(text)):
        if rng.random() < 0.7:
            text[i] = "ACGT"[rng.integers(0, 4)]
    # keep a few intact copies so that some windows do hit
    for at in (1500, 9000, 16500):
        text[at : at + len(cons)] = cons
    reads = [(7, "".join(text)), (8, cons[:100]), (9, "ACGTN" * 50)]
    rows = run_scan(str(tmp_path), reads)
    want = oracle_scan(orc, read_dcp(DCP), reads, True, False)
    assert rows == want
    assert any(r.split("\t")[1] != "0" for r in rows)  # a hit in a later window
    # dcp_scan_run scores every pair's no-hit chain in one launch and lets only the pairs that hit walk their real
    # chains; with nothing speculated -- every pair round by round -- the file is the same
    os.environ["DECIPHON_HIP_SPECULATE"] = "0"
    try:
        assert run_scan(str(tmp_path / "rounds"), reads) == rows
    finally:
        del os.environ["DECIPHON_HIP_SPECULATE"]


def test_long_reads_with_error_bearing_domains_like_config5(tmp_path, orc):
    """SURVEY 8(d) config 5 in small: 50 kb reads with planted domains carrying 12 % errors
    (8 % substitutions, 2 % insertions, 2 % deletions), about 7 chained windows per
    (profile, read) pair; every product row (window chain, hit span, lrt, every step of every
    path) against the oracle-driven restatement of thread_run."""
    rng = np.random.default_rng(59)
    cons = [t for _, t in read_fasta(os.path.join(GOLDEN, "consensus.fna"))]
    reads = []
    for sid in range(3):
        text = ["ACGT"[i] for i in rng.integers(0, 4, size=50000)]
        for at in sorted(rng.integers(0, 48000, size=7)):
            dom = []
            for ch in cons[int(rng.integers(0, len(cons)))]:
                u = rng.random()
                if u < 0.02:
                    continue
                if u < 0.04:
                    dom.append("ACGT"[rng.integers(0, 4)])
                dom.append("ACGT"[rng.integers(0, 4)] if rng.random() < 0.08 else ch)
            text[at : at + len(dom)] = dom
        reads.append((100 + sid, "".join(text[:50000])))
    rows = run_scan(str(tmp_path), reads)
    want = oracle_scan(orc, read_dcp(DCP), reads, True, False)
    assert rows == want
    assert len(rows) >= 10 and len({r.split("\t")[1] for r in rows}) >= 4  # hits in several windows of the chains


def test_partitions_concatenate_to_the_whole_scan(tmp_path, orc):
    """Contiguous profile partitions (c-core/partition_size.c) scanned separately give, in
    partition order, exactly the rows of the unpartitioned scan (c-core/product.c:63-81)."""
    named = read_fasta(os.path.join(GOLDEN, "consensus.fna"))
    reads = [(i, s) for i, (_, s) in enumerate(named)]
    whole = run_scan(str(tmp_path / "w"), reads)
    parts = []
    for idx in range(2):
        parts += run_scan(str(tmp_path / f"p{idx}"), reads, partition=(0, idx, 2))
    assert parts == whole
    more = []
    for idx in range(5):  # more partitions than profiles: the surplus ones are empty
        d = tmp_path / f"q{idx}"
        more += run_scan(str(d), reads, partition=(0, idx, 5)) if idx < 3 else []
    assert more == whole


def test_errors_and_interrupt(tmp_path):
    from deciphon_amd.scan import Batch, DeciphonError, Scan, Sequence

    with pytest.raises(DeciphonError) as e:
        Scan(str(tmp_path / "nope.dcp"), 0, 1, True, False, False)
    assert e.value.code == 21  # DCP_EOPENDB
    b = Batch()
    with pytest.raises(DeciphonError) as e:
        b.add(Sequence(1, "bad", "ACGTU"))
    assert e.value.code == 74  # DCP_ENUCLTSEQTU
    b.add(Sequence(2, "rna", "ACGUACGU"))
    with Scan(DCP, 0, 1, True, False, False) as scan:
        with pytest.raises(DeciphonError) as e:
            scan.run(str(tmp_path), b)
        assert e.value.code == 72  # DCP_EDBDNASEQRNA
    cons = read_fasta(os.path.join(GOLDEN, "consensus.fna"))[0][1]
    b = Batch()
    b.add(Sequence(3, "ok", cons))
    calls = []
    scan = Scan(DCP, 0, 1, True, False, False, on_window=lambda: calls.append(1))
    with scan:
        scan.run(str(tmp_path), b)
        assert len(calls) == 3  # one callback per window: 3 profiles x 1 read x 1 window


def test_two_ranks_scan_their_partitions_and_gather(tmp_path):
    """deciphon_amd.dist.scan_partitioned under torchrun with 2 ranks (both on this box's one GPU,
    rows gathered over gloo): the gathered products.tsv equals the single-process scan's."""
    import subprocess
    import sys

    from dcp_testlib import ROOT

    reads = read_fasta(os.path.join(GOLDEN, "consensus_multi.fna"))
    fasta = tmp_path / "reads.fna"
    fasta.write_text("".join(f">r{i}\n{t}\n" for i, (_, t) in enumerate(reads)))
    single = run_scan(str(tmp_path / "single"), [(i, t) for i, (_, t) in enumerate(reads)])
    env = dict(os.environ, DECIPHON_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", "29533",
                        os.path.join(ROOT, "scripts", "scan_multi_gpu.py"), DCP, str(fasta), str(tmp_path / "multi")],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = (tmp_path / "multi" / "products.tsv").read_text().splitlines()
    assert lines[1:] == single and len(single) > 0


def test_speculative_chains_with_hits_all_along_long_reads(tmp_path, orc):
    """dcp_scan_run scores every pair's NO-hit window chain in one batch and lets the pairs that did hit walk their real
    chains: the windows after a hit keep their speculated scores only while they are the same windows (c-core/window.c:21-31
    moves the next window's start by the hit's end unless that lies more than 4 K before the window's end), the others are
    scored again in later rounds.  Short real-structured profiles (windows of 1500...8650 nt) against 30 kb reads that
    carry a domain every ~700 nt, so that hits fall at every offset of their windows, many pairs hit several times in a
    row and some windows must be re-scored -- every row against the oracle-driven thread_run, and the same file with
    nothing speculated (every pair round by round)."""
    from deciphon_amd import synth
    from deciphon_amd.scan import Batch, Scan, Sequence

    seeds = synth.load_seeds(DCP)
    Ks = (30, 45, 60, 93, 124, 173)
    prots = [synth.tile_protein(seeds, K, 29 * i, f"SP{K}") for i, K in enumerate(Ks)]
    dcp = str(tmp_path / "short.dcp")
    synth.write_dcp(dcp, prots, 0.01, False, False)
    rng = np.random.default_rng(2025)
    reads = []
    for sid in range(3):
        x = rng.integers(0, 4, size=30000).astype(np.uint8)
        at = int(rng.integers(0, 300))
        while at < 29000:
            p = prots[int(rng.integers(0, len(prots)))]
            dom = synth.mutate(synth.back_translate(p["consensus"]), rng, 0.03, 0.01, 0.01)
            dom = dom[: 30000 - at]
            x[at : at + len(dom)] = dom
            at += len(dom) + int(rng.integers(100, 900))
        reads.append((sid + 1, "".join("ACGT"[v] for v in x)))
    batch = Batch()
    for sid, text in reads:
        batch.add(Sequence(sid, f"r{sid}", text))
    with Scan(dcp, 0, 1, True, False, False) as scan:
        scan.run(str(tmp_path / "spec"), batch)
        rows = scan.products()
        timing = scan.last_timing()
    want = oracle_scan(orc, read_dcp(dcp), reads, True, False)
    assert rows == want
    assert len(rows) >= 60 and len({r.split("\t")[1] for r in rows}) >= 8  # hits in many windows of the chains
    assert timing["rounds"] >= 3 and timing["path_passes"] >= len(rows)  # windows were scored again after hits
    os.environ["DECIPHON_HIP_SPECULATE"] = "0"
    try:
        assert run_scan(str(tmp_path / "rounds"), reads, dbfile=dcp) == rows
    finally:
        del os.environ["DECIPHON_HIP_SPECULATE"]
    # ... and with many small cost batches in flight (chunks of 2e6 cells)
    os.environ["DECIPHON_HIP_CHUNK_CELLS"] = "2e6"
    try:
        assert run_scan(str(tmp_path / "chunks"), reads, dbfile=dcp) == rows
    finally:
        del os.environ["DECIPHON_HIP_CHUNK_CELLS"]


def long_read_case(tmp_path):
    """Profiles tiled from minifam with K = 3 ... 173 (the K = 12 tile hits tandem copies of its consensus, the K = 3
    one a few chance matches) and reads of 0.4 Mb carrying a planted domain every ~50 kb, with 10 kb reads of two other
    lengths in between, so that the chains of one profile are made for one length, another, and the first again.
    (0.4 Mb, not more: the oracle's scalar DP takes ~0.25 us a cell, and the K = 173 pair of one such read is ~20 s.)"""
    from deciphon_amd import synth

    seeds = synth.load_seeds(DCP)
    tiles = ((30, 0), (3, 234), (173, 74), (12, 498), (124, 148), (60, 185))  # (K, offset in the ring of nodes)
    prots = [synth.tile_protein(seeds, K, off, f"LR{K}") for K, off in tiles]
    dcp = str(tmp_path / "long_reads.dcp")
    synth.write_dcp(dcp, prots, 0.01, False, False)
    rng = np.random.default_rng(1505)
    reads = []
    for sid, n in enumerate((400_000, 10_000, 400_000, 9_990, 380_000)):
        x = rng.integers(0, 4, size=n).astype(np.uint8)
        at = int(rng.integers(0, 20_000)) if n > 100_000 else n
        while at < n - 3000:
            p = prots[int(rng.integers(0, len(prots)))]
            dom = synth.back_translate(p["consensus"])
            # the K = 12 tile only hits runs of copies of its consensus
            dom = np.concatenate([dom] * 20) if p["core_size"] < 30 else synth.mutate(dom, rng, 0.03, 0.01, 0.01)
            dom = dom[: n - at]
            x[at : at + len(dom)] = dom
            at += len(dom) + int(rng.integers(40_000, 60_000))
        reads.append((sid + 1, "".join("ACGT"[v] for v in x)))
    return dcp, reads


def oracle_scan_pairs(orc, db, reads, threads=16):
    """dcp_testlib.oracle_scan with one task per (profile, read) pair, rows in the reference's order."""
    from concurrent.futures import ThreadPoolExecutor

    tasks = [([prot], [read]) for prot in db.proteins for read in reads]
    with ThreadPoolExecutor(max(1, min(threads, os.cpu_count() or 1))) as ex:
        parts = list(ex.map(lambda t: dcp_testlib.oracle_scan(orc, t[0], t[1], True, False), tasks))
    return [r for part in parts for r in part]


def test_long_reads_split_into_capped_chunks_and_drained_path_passes(tmp_path, orc, monkeypatch):
    """dcp_scan_run's chunk planner and path-pass drain at the sizes where they matter, scaled down by their knobs:
    DECIPHON_HIP_CHUNK_WINDOWS = 1500 splits the K = 3 and K = 12 profiles by reads, and one K = 3 pair of a 0.4 Mb
    read (2878 windows) is a chunk above the cap on its own; DECIPHON_HIP_PATH_DRAIN_HITS = 1 stops beginning chunks
    whenever more than one hit waits, so the path passes run between chunks.  Every row equals the oracle-driven thread_run, the
    scan with the default settings (one chunk, the path passes at the end) and the scan with nothing speculated."""
    from deciphon_amd import host
    from deciphon_amd.scan import Batch, Scan, Sequence

    dcp, reads = long_read_case(tmp_path)
    db = read_dcp(dcp)
    batch = Batch()
    for sid, text in reads:
        batch.add(Sequence(sid, f"seq{sid}", text))

    def scan(tag):
        with Scan(dcp, 0, 1, True, False, False) as s:
            s.run(str(tmp_path / tag), batch)
            assert s.progress() == 100  # every profile counted once, at its last chunk of reads
            rows = s.products()
            timing = s.last_timing()
        assert open(str(tmp_path / tag / "products.tsv")).read().splitlines()[1:] == rows
        return rows, timing

    monkeypatch.setenv("DECIPHON_HIP_CHUNK_WINDOWS", "1500")
    monkeypatch.setenv("DECIPHON_HIP_PATH_DRAIN_HITS", "1")
    rows, timing = scan("capped")
    # the plan the scan ran: as dcp_scan_plan_chunks makes it, and with the cap broken by single pairs only
    K = [p.core_size for p in db.proteins]
    R = [len(t) for _, t in reads]
    chunks, windows = host.plan_chunks(K, R, 1.0e10, float("inf"), 1 << 21, 1500)
    assert timing["chunks"] == len(chunks) > 6
    assert timing["largest_chunk_windows"] == int(windows.max()) == host.window_count(400_000, 3) > 1500
    assert all(w <= 1500 or (c[1] - c[0] == 1 and c[3] - c[2] == 1) for c, w in zip(chunks.tolist(), windows))
    assert sum(1 for c in chunks if c[1] - c[0] == 1 and c[3] - c[2] < len(reads)) >= 6  # K = 3 and 12 by reads
    assert timing["path_passes"] >= len(rows)
    want = oracle_scan_pairs(orc, db, reads)
    assert rows == want
    assert len(rows) >= 40 and len({r.split("\t")[7] for r in rows}) == 6
    # hits of the profiles split by reads in chunks that start past read 0 (K = 3: reads 4..4, K = 12: 4..4) or
    # hold several reads (K = 12: reads 0..3)
    assert {("5", "LR3"), ("3", "LR12"), ("5", "LR12")} <= {(r.split("\t")[0], r.split("\t")[7]) for r in rows}
    monkeypatch.delenv("DECIPHON_HIP_CHUNK_WINDOWS")
    monkeypatch.delenv("DECIPHON_HIP_PATH_DRAIN_HITS")
    default_rows, default_timing = scan("default")
    assert default_rows == rows
    assert default_timing["chunks"] == 1 and default_timing["largest_chunk_windows"] == int(windows.sum())
    # the drained scan ran its path passes between chunks: in more batches than the one that ran them at the end
    assert timing["path_batches"] > default_timing["path_batches"] >= 1
    monkeypatch.setenv("DECIPHON_HIP_SPECULATE", "0")
    assert run_scan(str(tmp_path / "rounds"), reads, dbfile=dcp) == rows
