"""CPU: the strip class (profiles beyond 4096 positions, StripWave) a block at a time, on the wave emulator
(tests/emul/emul_strip_blocks.cpp) against the oracle, bit for bit: checkpoints of the ring, Spre, X and Bz every
B rows, every block recomputed from its checkpoint into a table of dcp_block_slots rows that held NaN before
(so anything read outside a block's own rows shows in the bits), the traceback resumed from block to block, and
the trellis replayed from the same blocks."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from dcp_testlib import ROOT, bits, code_rows, pack_profile, random_seq, synth_profile

SHAPES = [(1, 1, 3), (2, 1, 2), (1, 2, 3), (2, 2, 2), (4, 2, 2), (1, 4, 2), (1, 1, 5), (2, 2, 3)]  # (Q, W, strips)
BLOCKS = [5, 10, 15, 20, 0]
GROUPS = [1, 2, 3]


@pytest.fixture(scope="module")
def emsb():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "emul"), "-f", "strip_blocks.mk"], check=True)
    lib = C.CDLL(os.path.join(ROOT, "tests", "emul", "libdcp_emul_strip_blocks.so"))
    lib.emul_strip_path_blocks.restype = C.c_int
    lib.emul_strip_replay_blocks.restype = C.c_int
    yield lib
    # no emulated kernel read a row beyond its resource: nothing relies on what the buffer range rule returns there
    # (lane_ops_emul.h, em_row_range_zeros; DESIGN.md, "the two lane vocabularies")
    lib.emul_row_range_zeros.restype = C.c_long
    assert lib.emul_row_range_zeros() == 0


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _case(rng, orc, it, quant):
    # the shape moves on by one every eight cases and the mode changes every eight: every shape meets every mode, every
    # block size and the long delete runs (every fourth case), and every mode meets the delete runs
    Q, W, S = SHAPES[(it + it // len(SHAPES)) % len(SHAPES)]
    KS = 64 * Q * W
    K = int(rng.integers(KS * (S - 1) + 1, KS * S + 1))
    if it % 7 == 0:
        K = KS * S  # no padding at all
    if it % 11 == 0:
        K = KS * (S - 1) + 1  # one position in the last strip
    prof = synth_profile(rng, K, quant, [0, 0.05][it % 2])
    if it % 4 == 0:  # long delete runs: across lanes, wavefronts and strips
        prof.trans[7, 1:] = np.float32(0.01)
        prof.trans[3, 1:] = np.float32(0.02)
    B = BLOCKS[it % len(BLOCKS)]
    G = GROUPS[it % len(GROUPS)]  # blocks side by side, as the engine takes them
    L = int(rng.integers(20, 71))
    seq = random_seq(rng, L)
    mode = (it // len(SHAPES)) % 4  # all four (multi_hits, hmmer3_compat) modes
    xt = orc.xtrans(max(L // 3, 1), mode & 1, mode >> 1)
    if quant:
        xt = (np.round(xt / quant) * quant).astype(np.float32)
    pool, pd = pack_profile(prof, Q, W, S)
    xt16 = np.zeros(16, np.float32)
    xt16[:13] = xt
    return prof, seq, xt, pool, pd, code_rows(seq), xt16, B, G, L, K, ((Q, W, S), mode, it % 4 == 0, B)


def test_strip_path_in_blocks(emsb, orc):
    """Score = viterbi_cost, steps = trellis_unzip of the oracle's trellis.  Continuous tables: the traceback's tie
    code (-2, the literal pass takes such a window) is rare -- at most 5 % of the cases may end in it."""
    rng = np.random.default_rng(77)
    N = 128
    multi = ties = 0
    seen, groups = set(), set()
    for it in range(N):
        prof, seq, xt, pool, pd, rows, xt16, B, G, L, K, what = _case(rng, orc, it, None)
        seen.add(what)
        groups.add((B, G))
        cap = 2 * L + 2 * K + 64
        buf = np.zeros(cap, np.uint32)
        score = C.c_float(0)
        n = emsb.emul_strip_path_blocks(_vp(pool), C.byref(pd), _vp(rows), L, _vp(xt16), B, G, _vp(buf), C.c_long(cap),
                                        C.byref(score))
        assert bits(score.value) == bits(orc.cost(prof, xt, seq)), (it, K, L, B)
        if n == -2:
            ties += 1
            continue
        assert n > 0, (it, K, L, B, n)
        _, xo, no = orc.path(prof, xt, seq)
        ids, sizes = orc.unzip(K, L, xo, no)
        w = buf[cap - n:]
        assert np.array_equal(w & 0xFFFF, ids.astype(np.uint32)) and np.array_equal(w >> 16, sizes.astype(np.uint32)), \
            (it, K, L, B)
        multi += B > 0 and L > B + 5
    assert N >= 120 and ties <= N * 5 // 100 and multi > N // 2, (N, ties, multi)
    # every shape with every mode, and with long delete runs
    assert {(s, m) for s, m, _, _ in seen} == {(s, m) for s in SHAPES for m in range(4)}
    assert {s for s, _, d, _ in seen if d} == set(SHAPES) and {m for _, m, d, _ in seen if d} == set(range(4))
    assert {(s, b) for s, _, _, b in seen} == {(s, b) for s in SHAPES for b in BLOCKS}
    assert groups == {(b, g) for b in BLOCKS for g in GROUPS}


def test_strip_trellis_replayed_in_blocks(emsb, orc):
    """Tie-rich tables (every cost a multiple of 1 or 4): every xnodes and nodes word of the trellis replayed block by
    block equals the oracle's.  No case is skipped."""
    rng = np.random.default_rng(78)
    multi = 0
    groups = set()
    for it in range(120):
        quant = [1.0, 4.0][it % 2]
        prof, seq, xt, pool, pd, rows, xt16, B, G, L, K, _ = _case(rng, orc, it, quant)
        groups.add((B, G))
        xn = np.full(L + 1, 0xFFFFFFFF, np.uint32)
        nd = np.full((L + 1) * K, 0xFFFF, np.uint16)
        score = C.c_float(0)
        assert emsb.emul_strip_replay_blocks(_vp(pool), C.byref(pd), _vp(rows), L, _vp(xt16), B, G, _vp(xn), _vp(nd),
                                             C.byref(score)) == 0
        s_o, xo, no = orc.path(prof, xt, seq)
        assert bits(score.value) == bits(s_o), (it, K, L, B)
        assert np.array_equal(xn, xo), (it, K, L, B, quant)
        assert np.array_equal(nd, no), (it, K, L, B, quant)
        multi += B > 0 and L > B + 5
    assert multi > 60
    assert groups == {(b, g) for b in BLOCKS for g in GROUPS}
