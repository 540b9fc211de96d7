"""CPU: the special transitions, trellis_unzip and the window walk against the REFERENCE's own code.  oracle/Makefile
`ref` compiles c-core/xtrans.c, trellis.c (+ xrealloc.c) and window.c unmodified, with oracle/imm_shim/ standing in for
the few imm interfaces they include; oracle/ref_glue.c drives them (ref_xtrans, ref_unzip, ref_windows).  What they
answered is recorded under tests/golden/ (make_golden.py): reference_walks.npz for xtrans and windows, and the paths
of synth_ties.npz, minifam_consensus.npz and reference_pins.npz (live_*) for trellis_unzip.  Every test checks the
product's host code (dcp_xtrans, dcp_trellis_unzip, dcp_window_next / dcp_window_count) and the oracle's restatement
against that record, and against the reference itself where oracle/_ref was built."""
import hashlib
import os
import sys

import numpy as np
import pytest

import deciphon_amd
from deciphon_amd import host
from dcp_testlib import GOLDEN, random_seq, read_fasta, synth_profile, walks_reflib

sys.path.insert(0, GOLDEN)
from make_golden import (MODES, WIN_POLICIES, XT_EDGES, XT_ROWS, live_cases, oracle_windows,  # noqa: E402
                         synth_case_params, synth_xt, window_cases, window_last_hit, window_positions)


@pytest.fixture(scope="module")
def ref():
    """The reference's xtrans.c, trellis.c and window.c (oracle/_ref) where they were built, else None."""
    return walks_reflib()


@pytest.fixture(scope="module")
def walks():
    return np.load(os.path.join(GOLDEN, "reference_walks.npz"))


def _same_bits(a, b) -> bool:
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _first_bad_row(a, b):
    rows = np.nonzero((np.asarray(a, np.float32).view(np.uint32) != np.asarray(b, np.float32).view(np.uint32)).any(1))[0]
    return int(rows[0]) if len(rows) else None


# ---- xtrans -----------------------------------------------------------------------------------------------------------
def test_xtrans_table_is_the_references(ref, orc, walks):
    """c-core/xtrans.c (xtrans_setup + xtrans_setup_viterbi, the 13 values handed to viterbi.c) against dcp_xtrans --
    what fills the engine's xt_table -- and orc_xtrans: bit for bit (+0 / -0 and +inf included) for every seq_size
    1 .. 33 334 (every row a window of up to 100 000 nt reads, plus one) in all four modes, and at edge lengths up to
    INT_MAX."""
    assert [tuple(int(v) for v in m) for m in walks["xt_modes"]] == list(MODES)
    assert int(walks["xt_rows"]) == XT_ROWS == 33334
    assert [int(v) for v in walks["xt_edges"]] == XT_EDGES and len(XT_EDGES) == 42
    sizes = range(1, XT_ROWS + 1)
    for m, (mh, h3) in enumerate(MODES):
        prod = np.stack([deciphon_amd.xtrans(s, mh, h3) for s in sizes])
        orcs = np.stack([orc.xtrans(s, mh, h3) for s in sizes])
        assert _same_bits(prod, orcs), (mh, h3, 1 + _first_bad_row(prod, orcs))
        if ref is not None:
            refs = np.stack([ref.xtrans(s, mh, h3) for s in sizes])
            assert _same_bits(prod, refs), (mh, h3, 1 + _first_bad_row(prod, refs))
        assert hashlib.sha256(prod.tobytes()).hexdigest() == str(walks["xt_sha256"][m]), (mh, h3)
        for j, s in enumerate(XT_EDGES):
            want = walks["xt_edge_bits"][m, j]
            assert _same_bits(deciphon_amd.xtrans(s, mh, h3), want.view(np.float32)), (mh, h3, s)
            assert _same_bits(orc.xtrans(s, mh, h3), want.view(np.float32)), (mh, h3, s)
            if ref is not None:
                assert _same_bits(ref.xtrans(s, mh, h3), want.view(np.float32)), (mh, h3, s)
    # the modes differ where they must: E -> J is closed without multi_hits, N -> N is free with hmmer3_compat
    e = walks["xt_edge_bits"].view(np.float32)
    assert np.isinf(e[1, :, 7]).all() and np.isfinite(e[0, :, 7]).all()  # EJ
    assert (e[2, :, 2] == 0).all() and (e[0, :8, 2] > 0).all()  # NN


# ---- trellis_unzip ----------------------------------------------------------------------------------------------------
def _unzips(orc, K, L, xn, nd, want, where):
    """orc.unzip and dcp_trellis_unzip of one trellis against the reference's path `want` (ids, sizes)."""
    for name, (ids, sizes) in (("oracle", orc.unzip(K, L, xn, nd)), ("product", host.unzip(K, L, xn, nd))):
        assert np.array_equal(ids, want[0]) and np.array_equal(sizes, want[1]), (name, *where)


def _golden_path(g, j, prefix=""):
    a, b = int(g[f"{prefix}path_off"][j]), int(g[f"{prefix}path_off"][j + 1])
    return g[f"{prefix}path_ids"][a:b], g[f"{prefix}path_sizes"][a:b]


def test_unzip_of_tie_rich_goldens(ref, orc):
    """The 240 tie-rich cases of synth_ties.npz (costs quantised to 0.5 .. 8: equal-cost predecessors everywhere):
    the paths the reference's trellis_unzip took through the reference's own trellises."""
    g = np.load(os.path.join(GOLDEN, "synth_ties.npz"))
    rng = np.random.default_rng(int(g["seed"]))
    walked = 0
    for it in range(int(g["ncase"])):
        K, L, quant, pinf, mh, h3 = synth_case_params(rng, it)
        prof = synth_profile(rng, K, quant, pinf)
        seq = random_seq(rng, L)
        want = _golden_path(g, it)
        alt = np.uint32(g["alt_bits"][it]).view(np.float32)
        if not np.isfinite(alt):  # no finite path: nothing was unzipped
            assert len(want[0]) == 0
            continue
        xt = synth_xt(orc, L, mh, h3, quant)
        _, xn, nd = orc.path(prof, xt, seq)
        _unzips(orc, K, L, xn, nd, want, (it, K, L))
        if ref is not None:
            ref.setup(prof)
            ref.path(xt, seq)
            got = ref.unzip(L)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (it, K, L)
        walked += 1
    assert walked >= 150 and int(g["path_off"][-1]) == len(g["path_ids"]) == len(g["path_sizes"])


def test_unzip_of_live_goldens(ref, orc):
    """The 330 cases of test_oracle.py::test_live_against_reference_viterbi (K up to 9000): reference_pins.npz live_*."""
    g = np.load(os.path.join(GOLDEN, "reference_pins.npz"))
    walked = 0
    for it, (prof, seq, xt) in enumerate(live_cases(orc)):
        want = _golden_path(g, it, "live_")
        if not np.isfinite(np.uint32(g["live_cost_bits"][it]).view(np.float32)):
            assert len(want[0]) == 0
            continue
        _, xn, nd = orc.path(prof, xt, seq)
        _unzips(orc, prof.K, len(seq), xn, nd, want, (it, prof.K))
        if ref is not None:
            ref.setup(prof)
            ref.path(xt, seq)
            got = ref.unzip(len(seq))
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (it, prof.K)
        walked += 1
    assert walked >= 250 and len(g["live_path_off"]) == 331


def test_unzip_of_minifam_goldens(ref, orc):
    """minifam.dcp x the consensus reads x the four modes (minifam_consensus.npz), every window that hits."""
    from oracle.dcp_reader import read_dcp

    g = np.load(os.path.join(GOLDEN, "minifam_consensus.npz"))
    profs = [orc.setup_profile(p) for p in read_dcp(os.path.join(GOLDEN, "minifam.dcp")).proteins]
    reads = read_fasta(os.path.join(GOLDEN, "consensus.fna")) + read_fasta(os.path.join(GOLDEN, "consensus_multi.fna"))
    walked = 0
    for j in range(len(g["profile"])):
        want = _golden_path(g, j)
        if len(want[0]) == 0:
            continue
        prof, x = profs[int(g["profile"][j])], orc.encode(reads[int(g["read"][j])][1])
        xt = orc.xtrans(max(len(x) // 3, 1), int(g["multi_hits"][j]), int(g["hmmer3_compat"][j]))
        _, xn, nd = orc.path(prof, xt, x)
        _unzips(orc, prof.K, len(x), xn, nd, want, (j,))
        if ref is not None:
            ref.setup(prof)
            ref.path(xt, x)
            got = ref.unzip(len(x))
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), j
        walked += 1
    assert walked >= 30


@pytest.mark.parametrize("quant", [0.5, 2.0, 8.0])
def test_unzip_of_fresh_tie_rich_cases(ref, orc, quant):
    """Fresh tie-rich cases over K = 2 .. 9000: each trellis walked by the reference's trellis_unzip (where oracle/_ref
    is built), dcp_trellis_unzip and orc.unzip.  Every reference run starts on a just-set-up struct viterbi
    (ref_fresh).  Windows whose score is +inf are left out: there is no path to walk."""
    rng = np.random.default_rng(int(quant * 16) + 7)
    Ks = (2, 3, 4, 5, 7, 8, 9, 16, 17, 33, 63, 64, 65, 128, 129, 255, 256, 257, 384, 385, 1000, 2049, 4096, 4097, 9000)
    walked = 0
    for it in range(100):
        K = int(Ks[it % len(Ks)])
        prof = synth_profile(rng, K, quant, [0.0, 0.05, 0.3][it % 3])
        seq = random_seq(rng, int(rng.integers(1, 90)))
        xt = synth_xt(orc, len(seq), it % 2, (it // 2) % 2, quant)
        score, xn, nd = orc.path(prof, xt, seq)
        if not np.isfinite(score):
            continue
        ids, sizes = orc.unzip(K, len(seq), xn, nd)
        want = (ids, sizes)
        if ref is not None:
            ref.setup(prof)
            rx, rn = ref.path(xt, seq)
            assert np.array_equal(rx, xn) and np.array_equal(rn, nd), (it, K)
            want = ref.unzip(len(seq))
        _unzips(orc, K, len(seq), xn, nd, want, (it, K, quant))
        walked += 1
    assert walked >= 60


# ---- windows ----------------------------------------------------------------------------------------------------------
def _product_windows(L, K, policy):
    w, out = host.WindowIter(L, K), []
    while (nxt := w.next()) is not None:
        idx, a, b = nxt
        out.append((a, b))
        p = window_last_hit(policy, idx, a, b)
        if p is not None:
            w.set_last_hit_position(p)
    return np.array(out, np.int32).reshape(-1, 2)


def test_window_walk_is_the_references(ref, orc, walks):
    """c-core/window.c (window_setup / window_next / window_set_last_hit_position) against dcp_window_next, the
    oracle's walk and -- for the chains without hits -- dcp_window_count, which the scan's chunk planner counts with.
    K around the 50 K = 100 000 switch and the strip class; reads at 1, 50 K +- 1, 100 000 +- 1, 120 000, 250 001; the
    last hit reported after each window at -1, 0, mid-window, the window's end - 1, or a mix."""
    cases = window_cases()
    assert [tuple(int(v) for v in c) for c in walks["win_cases"]] == cases and len(cases) == 180
    assert {WIN_POLICIES[p] for _, _, p in cases} == set(WIN_POLICIES)
    off, ranges = walks["win_off"], walks["win_ranges"]
    for i, (L, K, policy) in enumerate(cases):
        want = ranges[int(off[i]) : int(off[i + 1])]
        assert len(want) >= 1 and want[0][0] == 0 and want[-1][1] == L, (L, K, policy)
        assert np.array_equal(_product_windows(L, K, policy), want), (L, K, WIN_POLICIES[policy])
        assert np.array_equal(oracle_windows(orc, L, K, policy), want), (L, K, WIN_POLICIES[policy])
        if WIN_POLICIES[policy] in ("none", "-1", "0"):  # the same chain: a hit ending at 0 moves nothing
            assert host.window_count(L, K) == len(want), (L, K, WIN_POLICIES[policy])
        if ref is not None:
            pos = window_positions(policy, want)
            got = ref.windows(L, K, np.append(pos, np.int32(ref.NO_HIT)))
            assert np.array_equal(got, want), (L, K, WIN_POLICIES[policy])
