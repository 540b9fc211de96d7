"""GPU: the path pass of profiles beyond 4096 positions (strip class) a block at a time.  A window whose whole DP
table exceeds DECIPHON_HIP_PATH_BUDGET_MB is taken from checkpoints every DECIPHON_HIP_CKPT_ROWS rows, G blocks side by
side, fast pass and literal pass alike; one whose table fits keeps it.  Against the CPU oracle and the reference's own
bits (tests/golden/large_classes.npz, window_cap.npz).  The budgets are computed from the layout of
deciphon_amd/csrc/dcp_types.h (tests/path_layout.py) so that the blocks fit and the whole table does not; every budget is set on a fresh
Engine (its table arena holds nothing yet and never shrinks)."""
import os
import zlib

import numpy as np
import pytest

from dcp_testlib import GOLDEN, bits, synth_profile
from large_cases import build_case, large_cases, tiled_protein, window_cap_cases
from path_layout import MB, budget_mb, fast_bytes, fast_bytes_of, literal_bytes, table_bytes

pytestmark = pytest.mark.gpu

_oracle_paths = {}


def oracle_path(orc, key, prof, seq, mh=True, h3=False):
    """-> (score, state ids, emission lengths) of the CPU oracle, kept per case (K = 4200 x 3000 rows takes seconds)"""
    if key not in _oracle_paths:
        xt = orc.xtrans(max(len(seq) // 3, 1), mh, h3)
        score, xn, nd = orc.path(prof, xt, seq)
        ids, sizes = orc.unzip(prof.K, len(seq), xn, nd)
        _oracle_paths[key] = (score, ids, sizes)
    return _oracle_paths[key]


def same_path(p, want):
    score, ids, sizes = want
    return bits(p["score"]) == bits(score) and np.array_equal(p["state_ids"], ids) and np.array_equal(p["seqsizes"], sizes)


STRICT_CASE = dict(idx=102, K=4200, L=3000, kind="tiled", quant=None, pinf=0.0, mh=1, h3=0)  # test_gpu_large's


@pytest.mark.parametrize("B,G", [(50, 1), (500, 1), (50, 3), (500, 3)])
def test_a_table_beyond_the_budget_goes_in_blocks(orc, monkeypatch, B, G):
    """K = 4200 x 3000 rows (a whole table of 221 MB) under a budget that holds G block tables and the checkpoints:
    the oracle's score and steps, one window in blocks, never more placed than the budget.  Then, the budget raised
    above the whole table on the same engine: the whole table again, the same steps."""
    import deciphon_amd

    c = STRICT_CASE
    K, L = c["K"], c["L"]
    prof, seq, _ = build_case(c, orc)
    want = oracle_path(orc, "strict", prof, seq)
    budget = budget_mb(fast_bytes(L, K, B, G))
    assert fast_bytes(L, K, B, G) <= budget * MB < table_bytes(L, K)
    monkeypatch.delenv("DECIPHON_HIP_PATH_STRICT", raising=False)
    monkeypatch.delenv("DECIPHON_HIP_PATH", raising=False)
    monkeypatch.setenv("DECIPHON_HIP_CKPT_ROWS", str(B))
    monkeypatch.setenv("DECIPHON_HIP_PATH_GROUP", str(G))
    monkeypatch.setenv("DECIPHON_HIP_PATH_BUDGET_MB", str(budget))
    with deciphon_amd.Engine(0) as eng:
        eng.add_profile(prof.K, prof.trans, prof.match, prof.null, prof.bg)
        eng.commit()
        eng.set_sequences([seq])
        eng.set_mode(True, False)
        win = [(0, 0, 0, L)]
        p = eng.path(win, trellis=False)[0]
        print(f"B={B} G={G}: budget {budget} MB, placed {eng.path_table_bytes / MB:.1f} MB, blocked {eng.path_blocked}, "
              f"redone {eng.path_redone}")
        assert same_path(p, want)
        assert eng.path_blocked == 1
        assert 0 < eng.path_table_bytes <= budget * MB
        monkeypatch.setenv("DECIPHON_HIP_PATH_BUDGET_MB", str(budget_mb(table_bytes(L, K)) + 64))
        q = eng.path(win, trellis=False)[0]
        assert eng.path_blocked == 0
        assert eng.path_table_bytes >= table_bytes(L, K)
        assert same_path(q, want)


@pytest.mark.parametrize("idx", [30, 31])
def test_10_kb_reads_against_reference_goldens_in_blocks(orc, monkeypatch, idx):
    """SURVEY 3b, K = 8192 and 16383 on 10 kb reads (reference viterbi.c bits) under a budget below their whole
    tables (0.98 and 1.97 GB): score bits and the unzipped path of the fast pass; then the trellis -- the literal pass,
    replayed block by block from the same checkpoints with a block's rows of scratch -- by CRC32, and its path; the
    bytes placed stay within the budget through both."""
    import deciphon_amd

    g = np.load(os.path.join(GOLDEN, "large_classes.npz"))
    c = large_cases()[idx]
    K, L, B = c["K"], c["L"], 500
    assert K in (8192, 16383) and L == 10000 and (K, L) == (int(g["K"][idx]), int(g["L"][idx]))
    prof, seq, _ = build_case(c, orc)
    budget = budget_mb(literal_bytes(L, K, B, 1))
    assert budget * MB < table_bytes(L, K)
    for name in ("DECIPHON_HIP_PATH_STRICT", "DECIPHON_HIP_PATH", "DECIPHON_HIP_CKPT_ROWS", "DECIPHON_HIP_PATH_GROUP"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("DECIPHON_HIP_PATH_BUDGET_MB", str(budget))
    a, b = int(g["path_off"][idx]), int(g["path_off"][idx + 1])
    assert b > a
    with deciphon_amd.Engine(0) as eng:
        eng.add_profile(prof.K, prof.trans, prof.match, prof.null, prof.bg)
        eng.commit()
        eng.set_sequences([seq])
        eng.set_mode(bool(c["mh"]), bool(c["h3"]))
        win = [(0, 0, 0, L)]
        p = eng.path(win, trellis=False)[0]
        print(f"K={K}: budget {budget} MB, fast pass placed {eng.path_table_bytes / MB:.1f} MB, redone {eng.path_redone}")
        assert bits(p["score"]) == int(g["alt_bits"][idx])
        assert np.array_equal(p["state_ids"], g["path_ids"][a:b]) and np.array_equal(p["seqsizes"], g["path_sizes"][a:b])
        assert eng.path_blocked == 1
        assert 0 < eng.path_table_bytes <= budget * MB
        p = eng.path(win, trellis=True)[0]
        print(f"K={K}: with the trellis placed {eng.path_table_bytes / MB:.1f} MB")
        assert zlib.crc32(p["xnodes"].tobytes()) == int(g["xnodes_crc"][idx])
        assert zlib.crc32(p["nodes"].tobytes()) == int(g["nodes_crc"][idx])
        assert bits(p["literal_score"]) == int(g["alt_bits"][idx])
        assert np.array_equal(p["literal_state_ids"], g["path_ids"][a:b])
        assert np.array_equal(p["literal_seqsizes"], g["path_sizes"][a:b])
        assert eng.path_blocked == 1
        assert eng.path_table_bytes <= budget * MB


def test_whole_tables_blocks_and_short_profiles_in_one_request(orc, monkeypatch):
    """One dcp_hip_path with a strip window whose table fits the budget (600 rows, 44 MB), one whose table does not
    (3000 rows, 221 MB) and a window of a profile of 300 positions: all three equal the oracle, one went in blocks --
    and so do their trellises (the literal pass of the same mix)."""
    import deciphon_amd

    c = STRICT_CASE
    K, L, B = c["K"], c["L"], 500
    prof, seq, _ = build_case(c, orc)
    small = synth_profile(np.random.default_rng(5), 300)
    short = 600
    budget = 160
    assert table_bytes(short, K) + literal_bytes(L, K, B, 1) + 8 * MB < budget * MB < table_bytes(L, K)
    for name in ("DECIPHON_HIP_PATH_STRICT", "DECIPHON_HIP_PATH", "DECIPHON_HIP_CKPT_ROWS", "DECIPHON_HIP_PATH_GROUP"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("DECIPHON_HIP_PATH_BUDGET_MB", str(budget))
    wins = [(0, 0, 0, short), (1, 0, 100, 2100), (0, 0, 0, L)]
    profs = [prof, small, prof]
    want = [oracle_path(orc, "strict-short", prof, np.ascontiguousarray(seq[:short])),
            oracle_path(orc, "small", small, np.ascontiguousarray(seq[100:2100])),
            oracle_path(orc, "strict", prof, seq)]
    with deciphon_amd.Engine(0) as eng:
        eng.add_profile(prof.K, prof.trans, prof.match, prof.null, prof.bg)
        eng.add_profile(small.K, small.trans, small.match, small.null, small.bg)
        eng.commit()
        eng.set_sequences([seq])
        eng.set_mode(True, False)
        res = eng.path(wins, trellis=False)
        print(f"mixed: placed {eng.path_table_bytes / MB:.1f} MB of {budget} MB, blocked {eng.path_blocked}")
        for r, w in zip(res, want):
            assert same_path(r, w)
        assert eng.path_blocked == 1
        assert eng.path_table_bytes <= budget * MB
        res = eng.path(wins, trellis=True)
        for (pi, si, a, b), r, pf, w in zip(wins, res, profs, want):
            x = np.ascontiguousarray(seq[a:b])
            _, xn, nd = orc.path(pf, orc.xtrans(max(len(x) // 3, 1), True, False), x)
            assert np.array_equal(r["xnodes"], xn) and np.array_equal(r["nodes"], nd), (pi, a, b)
            assert bits(r["literal_score"]) == bits(w[0])
            assert np.array_equal(r["literal_state_ids"], w[1]) and np.array_equal(r["literal_seqsizes"], w[2])
        assert eng.path_table_bytes <= budget * MB


def test_a_window_at_the_cap_under_the_default_budget(orc, monkeypatch):
    """K = 4200 x 100 000 rows (tests/golden/window_cap.npz) on a fresh engine with nothing set: the whole table
    (7.4 GB by the layout) is beyond the default budget, so the window goes in blocks -- golden score and path, less
    placed than the whole table and at most 16 GB."""
    import deciphon_amd

    g = np.load(os.path.join(GOLDEN, "window_cap.npz"))
    c = window_cap_cases()[1]
    K, L = c["K"], c["L"]
    assert (K, L) == (4200, 100000) == (int(g["K"][1]), int(g["L"][1]))
    for name in ("DECIPHON_HIP_PATH_STRICT", "DECIPHON_HIP_PATH", "DECIPHON_HIP_CKPT_ROWS", "DECIPHON_HIP_PATH_GROUP",
                 "DECIPHON_HIP_PATH_BUDGET_MB"):
        monkeypatch.delenv(name, raising=False)
    prof, seq, _ = build_case(c, orc)
    a, b = int(g["path_off"][1]), int(g["path_off"][2])
    with deciphon_amd.Engine(0) as eng:
        eng.add_profile(prof.K, prof.trans, prof.match, prof.null, prof.bg)
        eng.commit()
        eng.set_sequences([seq])
        eng.set_mode(True, False)
        p = eng.path([(0, 0, 0, L)], trellis=False)[0]
        print(f"window cap: placed {eng.path_table_bytes / 1e9:.2f} GB, whole table {table_bytes(L, K) / 1e9:.2f} GB")
        assert bits(p["score"]) == int(g["alt_bits"][1])
        assert np.array_equal(p["state_ids"], g["path_ids"][a:b]) and np.array_equal(p["seqsizes"], g["path_sizes"][a:b])
        assert eng.path_blocked == 1
        assert 0 < eng.path_table_bytes < table_bytes(L, K)
        assert eng.path_table_bytes <= 16 << 30


def test_scan_of_a_30_kb_read_under_a_small_budget(tmp_path, orc, monkeypatch):
    """Through dcp_scan_run: a one-profile database with K = 4200 against a 30 kb read that carries the profile's
    back-translated consensus, DECIPHON_HIP_PATH_BUDGET_MB far below the window's table (30 001 rows, 2.2 GB): every
    row equals the oracle-driven thread_run."""
    from dcp_testlib import oracle_scan
    from deciphon_amd import synth
    from deciphon_amd.scan import Batch, Scan, Sequence
    from oracle.dcp_reader import read_dcp

    c = STRICT_CASE
    n = 30000
    budget = 256
    assert literal_bytes(n, c["K"], 500, 1) < budget * MB < table_bytes(n, c["K"])
    for name in ("DECIPHON_HIP_PATH_STRICT", "DECIPHON_HIP_PATH", "DECIPHON_HIP_CKPT_ROWS", "DECIPHON_HIP_PATH_GROUP"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("DECIPHON_HIP_PATH_BUDGET_MB", str(budget))
    rng = np.random.default_rng(9)
    read = rng.integers(0, 4, size=n).astype(np.uint8)
    dom = synth.back_translate(tiled_protein(c)["consensus"])
    assert 5000 + len(dom) < n
    read[5000 : 5000 + len(dom)] = dom
    text = "".join("ACGT"[v] for v in read)
    dcp = str(tmp_path / "k4200.dcp")
    synth.write_dcp(dcp, [tiled_protein(c)], 0.01, False, False)
    batch = Batch()
    batch.add(Sequence(7, "read", text))
    with Scan(dcp, 0, 1, True, False, False) as scan:
        scan.run(str(tmp_path / "prod"), batch)
        rows = scan.products()
    want = oracle_scan(orc, read_dcp(dcp).proteins, [(7, text)], True, False)
    assert len(want) >= 1 and rows == want


def test_the_literal_pass_alone_counts_its_blocks(orc, monkeypatch):
    """DECIPHON_HIP_PATH=literal skips the fast pass: the window whose table + scratch exceed the budget is replayed
    block by block, counted by path_blocked, within the budget, and gives the oracle's steps."""
    import deciphon_amd

    c = STRICT_CASE
    K, L, B = c["K"], c["L"], 500
    prof, seq, _ = build_case(c, orc)
    want = oracle_path(orc, "strict", prof, seq)
    budget = budget_mb(literal_bytes(L, K, B, 1))
    assert budget * MB < table_bytes(L, K)
    for name in ("DECIPHON_HIP_PATH_STRICT", "DECIPHON_HIP_CKPT_ROWS", "DECIPHON_HIP_PATH_GROUP"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("DECIPHON_HIP_PATH", "literal")
    monkeypatch.setenv("DECIPHON_HIP_PATH_BUDGET_MB", str(budget))
    with deciphon_amd.Engine(0) as eng:
        eng.add_profile(prof.K, prof.trans, prof.match, prof.null, prof.bg)
        eng.commit()
        eng.set_sequences([seq])
        eng.set_mode(True, False)
        p = eng.path([(0, 0, 0, L)], trellis=False)[0]
        assert same_path(p, want)
        assert eng.path_redone == 1 and eng.path_blocked == 1
        assert 0 < eng.path_table_bytes <= budget * MB


@pytest.mark.parametrize("G", [1, 2, 3])
@pytest.mark.parametrize("mode", ["fast", "literal"])
def test_the_bytes_placed_are_the_layouts(orc, monkeypatch, mode, G):
    """K = 4200 x 120 rows in blocks of 50: three blocks, the smallest window that has them.  The budget holds one block
    table and the checkpoints and not the whole table (8.9 MB), so the window goes in blocks; G of them side by side are
    what DECIPHON_HIP_PATH_GROUP says, and beyond G = 1 they pass the budget as the lone placement of a slice does.  The
    bytes placed are exactly the layout's: G tables and the checkpoints in the fast pass, and with the replay scratch
    of G blocks when DECIPHON_HIP_PATH=literal skips it."""
    import deciphon_amd

    K, L, B = STRICT_CASE["K"], 120, 50
    prof, seq, _ = build_case(STRICT_CASE, orc)
    seq = np.ascontiguousarray(seq[:L])
    want = oracle_path(orc, "strict-120", prof, seq)
    budget = budget_mb(fast_bytes(L, K, B, 1))
    assert fast_bytes(L, K, B, 1) <= budget * MB < table_bytes(L, K)
    monkeypatch.delenv("DECIPHON_HIP_PATH_STRICT", raising=False)
    monkeypatch.delenv("DECIPHON_HIP_PATH", raising=False)
    if mode == "literal":
        monkeypatch.setenv("DECIPHON_HIP_PATH", "literal")
    monkeypatch.setenv("DECIPHON_HIP_CKPT_ROWS", str(B))
    monkeypatch.setenv("DECIPHON_HIP_PATH_GROUP", str(G))
    monkeypatch.setenv("DECIPHON_HIP_PATH_BUDGET_MB", str(budget))
    with deciphon_amd.Engine(0) as eng:
        eng.add_profile(prof.K, prof.trans, prof.match, prof.null, prof.bg)
        eng.commit()
        eng.set_sequences([seq])
        eng.set_mode(True, False)
        p = eng.path([(0, 0, 0, L)], trellis=False)[0]
        print(f"{mode} G={G}: placed {eng.path_table_bytes}, fast {fast_bytes(L, K, B, G)}, literal {literal_bytes(L, K, B, G)}, "
              f"blocked {eng.path_blocked}, redone {eng.path_redone}")
        assert same_path(p, want)
        assert eng.path_blocked == 1
        assert eng.path_redone == (1 if mode == "literal" else 0)
        assert eng.path_table_bytes == (literal_bytes if mode == "literal" else fast_bytes)(L, K, B, G)


def test_the_bytes_placed_for_a_short_profile_are_the_layouts(orc, monkeypatch):
    """K = 300 (384 padded positions on one wavefront) x 120 rows in blocks of 50, two side by side: two block tables
    and the two checkpoints of the class's own size, rounded up to 256 bytes."""
    import deciphon_amd

    L, B, G = 120, 50, 2
    small = synth_profile(np.random.default_rng(5), 300)
    seq = np.ascontiguousarray(build_case(STRICT_CASE, orc)[1][100 : 100 + L])
    want = oracle_path(orc, "small-120", small, seq)
    for name in ("DECIPHON_HIP_PATH_STRICT", "DECIPHON_HIP_PATH", "DECIPHON_HIP_PATH_BUDGET_MB"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("DECIPHON_HIP_CKPT_ROWS", str(B))
    monkeypatch.setenv("DECIPHON_HIP_PATH_GROUP", str(G))
    with deciphon_amd.Engine(0) as eng:
        eng.add_profile(small.K, small.trans, small.match, small.null, small.bg)
        eng.commit()
        eng.set_sequences([seq])
        eng.set_mode(True, False)
        p = eng.path([(0, 0, 0, L)], trellis=False)[0]
        print(f"K=300: placed {eng.path_table_bytes}, layout {fast_bytes_of(L, 384, 1, B, G, False)}, redone {eng.path_redone}")
        assert same_path(p, want)
        assert eng.path_blocked == 0 and eng.path_redone == 0
        assert eng.path_table_bytes == fast_bytes_of(L, 384, 1, B, G, False)
