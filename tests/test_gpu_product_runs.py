"""GPU: dcp_scan_run with its product rows going through sorted run files (DECIPHON_HIP_PRODUCT_MB, csrc/product_runs.h)
writes the products.tsv of the scan that holds every row in memory -- the default, whose rows tests/test_gpu_scan.py
pins to the oracle and to the reference's committed products.tsv -- holds less row text than that scan, and leaves
nothing but products.tsv in the product directory: finished, interrupted, or run a second time."""
import os

import numpy as np
import pytest

from dcp_testlib import GOLDEN, read_fasta

pytestmark = pytest.mark.gpu

DCP = os.path.join(GOLDEN, "minifam.dcp")
HEADER = "sequence\twindow\twindow_start\twindow_stop\thit\thit_start\thit_stop\tprofile\tabc\tlrt\tevalue\tmatch\n"


def make_batch(reads):
    from deciphon_amd.scan import Batch, Sequence

    batch = Batch()
    for sid, text in reads:
        batch.add(Sequence(sid, f"r{sid}", text))
    return batch


def scan_once(dcp, batch, out, **kw):
    """-> (bytes of products.tsv, products(), product_stats(), last_timing(), names in the product directory)"""
    from deciphon_amd.scan import Scan

    with Scan(dcp, 0, 1, True, False, False, **kw) as scan:
        scan.run(str(out), batch)
        got = scan.products(), scan.product_stats(), scan.last_timing()
    return (open(os.path.join(out, "products.tsv"), "rb").read(), *got, sorted(os.listdir(out)))


def row_bytes(rows):
    return sum(len(r.encode()) for r in rows)


@pytest.fixture(scope="module")
def hit_rich(tmp_path_factory):
    """The case of test_gpu_scan.py::test_speculative_chains_with_hits_all_along_long_reads: six profiles tiled from
    minifam, K = 30 ... 173, against three 30 kb reads that carry a domain every ~700 nt (seed 2025); and its scan at
    the default budget, the reference of this file."""
    from deciphon_amd import synth

    tmp = tmp_path_factory.mktemp("hit_rich")
    seeds = synth.load_seeds(DCP)
    Ks = (30, 45, 60, 93, 124, 173)
    prots = [synth.tile_protein(seeds, K, 29 * i, f"SP{K}") for i, K in enumerate(Ks)]
    dcp = str(tmp / "short.dcp")
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
    assert "DECIPHON_HIP_PRODUCT_MB" not in os.environ
    file, rows, stats, timing, names = scan_once(dcp, make_batch(reads), tmp / "default")
    return dict(dcp=dcp, reads=reads, Ks=Ks, file=file, rows=rows, stats=stats, timing=timing, names=names)


def spill_every_batch(monkeypatch):
    """Budget 0: the rows of every path batch are a run.  Chunks of 2e6 cells and a drain after every hit: path passes
    run between the chunks, so rows of late profiles are on disk before the follow-up rows of early ones arrive."""
    monkeypatch.setenv("DECIPHON_HIP_PRODUCT_MB", "0")
    monkeypatch.setenv("DECIPHON_HIP_CHUNK_CELLS", "2e6")
    monkeypatch.setenv("DECIPHON_HIP_PATH_DRAIN_HITS", "1")


def test_spilled_scan_writes_the_file_of_the_scan_that_held_every_row(tmp_path, hit_rich, monkeypatch):
    d = hit_rich
    assert d["file"].decode() == HEADER + "".join(r + "\n" for r in d["rows"])
    assert len(d["rows"]) >= 60 and d["timing"]["rounds"] >= 3  # windows were scored again after hits
    assert d["stats"] == dict(rows=len(d["rows"]), runs=0, peak_bytes=row_bytes(d["rows"]), file_bytes=len(d["file"]))
    assert d["names"] == ["products.tsv"]
    spill_every_batch(monkeypatch)
    file, rows, stats, timing, names = scan_once(d["dcp"], make_batch(d["reads"]), tmp_path / "spilled")
    print("default", d["stats"], "path batches", d["timing"]["path_batches"])
    print("spilled", stats, "path batches", timing["path_batches"])
    assert file == d["file"]
    assert rows == d["rows"]
    assert timing["path_batches"] >= 2
    assert stats["runs"] >= 2
    assert stats["peak_bytes"] < row_bytes(d["rows"])
    assert stats["rows"] == len(rows) and stats["file_bytes"] == len(file)
    assert names == ["products.tsv"]


def test_golden_hits_at_budget_zero(tmp_path, monkeypatch):
    reads = [(i, s) for i, (_, s) in enumerate(read_fasta(os.path.join(GOLDEN, "consensus.fna")))]
    file, rows, stats, _, names = scan_once(DCP, make_batch(reads), tmp_path / "default")
    assert len(rows) == 3 and stats["runs"] == 0 and names == ["products.tsv"]
    monkeypatch.setenv("DECIPHON_HIP_PRODUCT_MB", "0")
    file0, rows0, stats0, _, names0 = scan_once(DCP, make_batch(reads), tmp_path / "spilled")
    assert file0 == file and rows0 == rows
    assert stats0["runs"] >= 1 and stats0["rows"] == 3 and stats0["file_bytes"] == len(file)
    assert names0 == ["products.tsv"]


@pytest.mark.filterwarnings("ignore::pytest.PytestUnraisableExceptionWarning")
def test_interrupted_scan_leaves_no_run_file(tmp_path, hit_rich, monkeypatch):
    """An on_window that raises interrupts the scan as python-core's does (python-core/deciphon_core/scan.py:12-15):
    run returns, the rows found so far are written, and no run file stays.  The case makes 195 callbacks for its
    no-hit chains, not thousands, so the callback does not count to a fixed number: it raises at the first call that
    finds a run file in the product directory -- rows are on disk then, and chunks are still to come."""
    from deciphon_amd import host
    from deciphon_amd.scan import Scan

    d = hit_rich
    spill_every_batch(monkeypatch)
    windows = sum(host.window_count(len(t), K) for K in d["Ks"] for _, t in d["reads"])
    out = tmp_path / "interrupted"
    calls, seen = [], []

    def on_window():
        calls.append(1)
        if not seen and any(f.startswith(".products.") for f in os.listdir(out)):
            seen.extend(os.listdir(out))
            raise RuntimeError("stop here")

    with Scan(d["dcp"], 0, 1, True, False, False, on_window=on_window) as scan:
        scan.run(str(out), make_batch(d["reads"]))
        rows, stats = scan.products(), scan.product_stats()
        assert scan.interrupted
    print("interrupted after", len(calls), "callbacks; no-hit chains", windows, "windows; saw", seen, stats)
    assert seen and len(calls) < windows
    assert sorted(os.listdir(out)) == ["products.tsv"]
    assert (out / "products.tsv").read_text() == HEADER + "".join(r + "\n" for r in rows)
    assert stats["runs"] >= 1 and stats["rows"] == len(rows)
    assert 0 < len(rows) < len(d["rows"]) and set(rows) <= set(d["rows"])


def test_second_run_on_the_same_scan(tmp_path, hit_rich, monkeypatch):
    from deciphon_amd.scan import Scan

    d = hit_rich
    spill_every_batch(monkeypatch)
    one = d["reads"][1:2]
    want = [r for r in d["rows"] if r.split("\t")[0] == str(one[0][0])]
    assert 0 < len(want) < len(d["rows"])
    with Scan(d["dcp"], 0, 1, True, False, False) as scan:
        scan.run(str(tmp_path / "first"), make_batch(d["reads"]))
        assert scan.products() == d["rows"]
        scan.run(str(tmp_path / "second"), make_batch(one))
        rows, stats = scan.products(), scan.product_stats()
    assert rows == want
    file = (tmp_path / "second" / "products.tsv").read_bytes()
    assert file.decode() == HEADER + "".join(r + "\n" for r in want)
    assert stats["rows"] == len(want) and stats["file_bytes"] == len(file)
    assert 1 <= stats["runs"] and stats["peak_bytes"] <= row_bytes(want)
    for tag in ("first", "second"):
        assert sorted(os.listdir(tmp_path / tag)) == ["products.tsv"]
