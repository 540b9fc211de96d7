"""CPU: the product rows of a scan in bounded memory (csrc/product_runs.h, through include/deciphon_host.h
dcp_product_runs_*).  Rows handed over in any order must come out exactly as a stable sort by (profile, seq, window)
orders them -- what dcp_scan_run wrote while it held every row -- whether they all stayed in memory, went through a
few sorted run files, or through more run files than the merge opens at once; the text held is bounded by the budget
plus the largest single add; and no run file outlives close, deletion or an error."""
import os
import subprocess

import numpy as np
import pytest

from dcp_testlib import ROOT
from deciphon_amd import HipError, host

HEADER = b"sequence\twindow\twindow_start\twindow_stop\thit\thit_start\thit_stop\tprofile\tabc\tlrt\tevalue\tmatch\n"
NROWS, NADDS = 2000, 300
EOPENTMP = 23


@pytest.fixture(scope="module")
def case():
    """2000 rows: keys out of 10 x 20 x 25 so that about a fifth repeat one seen before, texts of 0 ... 4000 bytes
    with the separators of the match column in them and four of 300 KB, cut into 300 adds of uneven size."""
    rng = np.random.default_rng(20251)
    keys = np.stack([rng.integers(0, 10, NROWS), rng.integers(0, 20, NROWS), rng.integers(0, 25, NROWS)], 1)
    alphabet = np.frombuffer(b"ACGTacgtMIDNJCBES0123456789.,;\t-", np.uint8)
    lengths = rng.integers(0, 4001, NROWS)
    lengths[[0, 777, 1500, NROWS - 1]] = 300_000
    lengths[[5, 900]] = 0
    texts = [alphabet[rng.integers(0, len(alphabet), int(n))].tobytes() for n in lengths]
    cuts = [0] + sorted((rng.choice(NROWS - 1, NADDS - 1, replace=False) + 1).tolist()) + [NROWS]
    adds = list(zip(cuts[:-1], cuts[1:]))
    sizes = [b - a for a, b in adds]
    assert len(adds) == NADDS and min(sizes) == 1 and sizes.count(1) >= 5 and max(sizes) >= 20
    distinct = len({tuple(k) for k in keys.tolist()})
    assert 0.1 * NROWS < NROWS - distinct < 0.3 * NROWS
    order = sorted(range(NROWS), key=lambda i: tuple(keys[i]))  # (stable)
    lines = [texts[i] for i in order]
    return dict(keys=keys, texts=texts, adds=adds, lines=lines, file=HEADER + b"".join(t + b"\n" for t in lines),
                total=int(lengths.sum()), largest_add=max(int(lengths[a:b].sum()) for a, b in adds))


def fill(runs, case):
    k, t = case["keys"], case["texts"]
    for a, b in case["adds"]:
        runs.add(k[a:b, 0], k[a:b, 1], k[a:b, 2], t[a:b])


@pytest.mark.parametrize("budget", [1 << 62, 64 << 10, 1, 0])
def test_rows_come_out_in_stable_order_within_the_budget(tmp_path, case, budget):
    runs = host.ProductRuns(tmp_path, budget)
    fill(runs, case)
    file = tmp_path / "products.tsv"
    runs.close(file)
    st = runs.stats()
    print(budget, st)
    assert file.read_bytes() == case["file"]
    assert len(runs) == st["rows"] == NROWS and st["file_bytes"] == len(case["file"])
    for i in np.random.default_rng(3).permutation(NROWS).tolist():
        assert runs.row(i) == case["lines"][i], i
    assert runs.row(-1) is None and runs.row(NROWS) is None
    # by design, not by measurement: what add holds when it returns is within the budget
    assert st["peak_bytes"] <= budget + case["largest_add"]
    if budget == 1 << 62:
        assert st["runs"] == 0 and st["peak_bytes"] == case["total"]
    elif budget == 64 << 10:
        assert st["runs"] >= 2
    else:
        assert st["runs"] >= NADDS > 64  # every add is a run, and the merge opens 64 at a time: it went in passes
    assert os.listdir(tmp_path) == ["products.tsv"]
    file.unlink()
    for i in (0, NROWS - 1, 777, 5, 1234):
        assert runs.row(i) == case["lines"][i]
    runs.free()
    assert os.listdir(tmp_path) == []


@pytest.mark.parametrize("budget", [1 << 62, 0])
def test_no_rows(tmp_path, budget):
    runs = host.ProductRuns(tmp_path, budget)
    runs.add([], [], [], [])
    runs.close(tmp_path / "products.tsv")
    assert (tmp_path / "products.tsv").read_bytes() == HEADER
    assert len(runs) == 0 and runs.row(0) is None
    assert runs.stats() == dict(rows=0, runs=0, peak_bytes=0, file_bytes=len(HEADER))
    assert os.listdir(tmp_path) == ["products.tsv"]


def test_deleted_without_close_leaves_nothing(tmp_path, case):
    runs = host.ProductRuns(tmp_path, 64 << 10)
    fill(runs, case)
    assert runs.stats()["runs"] >= 2
    left = os.listdir(tmp_path)
    assert left and all(f.startswith(".products.") and f.endswith(".run") for f in left)
    runs.free()
    assert os.listdir(tmp_path) == []


def test_first_error_sticks_and_nothing_is_left(tmp_path, case):
    gone = tmp_path / "gone"
    gone.mkdir()
    runs = host.ProductRuns(gone, 0)
    gone.rmdir()
    k, t = case["keys"], case["texts"]
    for a, b in case["adds"][:3]:  # the add that spills first, and every one after it
        with pytest.raises(HipError) as e:
            runs.add(k[a:b, 0], k[a:b, 1], k[a:b, 2], t[a:b])
        assert e.value.code == EOPENTMP
    gone.mkdir()  # (the directory coming back does not clear the error)
    with pytest.raises(HipError) as e:
        runs.add(k[:1, 0], k[:1, 1], k[:1, 2], t[:1])
    assert e.value.code == EOPENTMP
    with pytest.raises(HipError) as e:
        runs.close(gone / "products.tsv")
    assert e.value.code == EOPENTMP
    assert len(runs) == 0 and runs.row(0) is None
    runs.free()
    assert os.listdir(gone) == []


def test_product_runs_under_sanitizers(tmp_path):
    """csrc/product_runs.cpp built with -fsanitize=address,undefined into a program of its own (tests/c/
    product_runs_sanitize.cpp): adds from two threads at budgets of 0 and 64 KB, the merge in passes, row() over every
    row, and destruction before close."""
    csrc = os.path.join(ROOT, "deciphon_amd", "csrc")
    exe = str(tmp_path / "product_runs_sanitize")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
                    "-I", csrc, "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c", "product_runs_sanitize.cpp"),
                    os.path.join(csrc, "product_runs.cpp"), "-o", exe], check=True)
    work = tmp_path / "prod"
    work.mkdir()
    r = subprocess.run([exe, str(work)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "product runs done" in r.stdout
    assert os.listdir(work) == []
