"""CPU: the windows of tests/block_edge_cases.py through the path pass in blocks on the wave emulator
(tests/emul/block_walk.h: the kernels' own CostWave / StripWave, dcp_traceback_group and the geometry of dcp_types.h),
against the oracle, step for step -- every class of the path pass, B = 5, 10, 20, one to three blocks side by side.  Every
run has a step buffer of exactly the path's N steps inside an array of sentinel words, so the upper limit of
traceback.h (`n + 1 >= cap`) is met in every window; a subset runs again at N - 1.  What the table must contain at the
block boundaries is asserted here (block_edge_cases.coverage), and which candidates tie is decided here too."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import block_edge_cases as bec
from dcp_testlib import ROOT, bits, code_rows, pack_profile
from path_layout import block, num_blocks

DCP_TB_OVERFLOW, DCP_TB_TIE = -1, -2  # deciphon_amd/csrc/traceback.h
SENTINEL = np.uint32(0xA5C3F00D)
GUARD = 16  # sentinel words on either side of a step buffer


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


class Emulator:
    def __init__(self):
        here = os.path.join(ROOT, "tests", "emul")
        subprocess.run(["make", "-s", "-C", here], check=True)
        subprocess.run(["make", "-s", "-C", here, "-f", "strip_blocks.mk"], check=True)
        self.cost = C.CDLL(os.path.join(here, "libdcp_emul.so"))
        self.strip = C.CDLL(os.path.join(here, "libdcp_emul_strip_blocks.so"))
        for lib in (self.cost, self.strip):
            lib.emul_row_range_zeros.restype = C.c_long
        self.cost.emul_path_blocks.restype = C.c_int
        self.strip.emul_strip_path_blocks.restype = C.c_int
        self.packed = {}

    def layout(self, pi):
        """the profile in the layout of its class; the strip class in the emulator's own strips (K > 4096: strips of
        512 positions on two wavefronts -- the steps and the tie do not depend on the shape)"""
        if pi not in self.packed:
            p = bec.profiles()[pi]
            shape = p.emul or ((4, 2, (p.K + 511) // 512) if p.cls == bec.STRIP else p.cls)
            self.packed[pi] = pack_profile(p.prof, *shape)
        return self.packed[pi]

    def path(self, orc, c, G, cap):
        """-> (what dcp_traceback returned, score, the buffer, the sentinels around it intact)"""
        p, seq = bec.window(c)
        pool, pd = self.layout(c.pi)
        xt16 = np.zeros(16, np.float32)
        xt16[:13] = bec.xt_of(orc, c.L)
        arr = np.full(cap + 2 * GUARD, SENTINEL, np.uint32)
        buf = arr[GUARD : GUARD + cap]
        score = C.c_float(0)
        f = self.strip.emul_strip_path_blocks if p.cls == bec.STRIP else self.cost.emul_path_blocks
        n = f(_vp(pool), C.byref(pd), _vp(code_rows(seq)), c.L, _vp(xt16), c.B, G, _vp(buf), C.c_long(cap), C.byref(score))
        intact = bool(np.all(arr[:GUARD] == SENTINEL) and np.all(arr[GUARD + cap :] == SENTINEL))
        return n, np.float32(score.value), buf, intact


@pytest.fixture(scope="module")
def emul():
    e = Emulator()
    yield e
    # no emulated kernel read a row beyond its resource (lane_ops_emul.h, em_row_range_zeros)
    assert e.cost.emul_row_range_zeros() == 0 and e.strip.emul_row_range_zeros() == 0


@pytest.fixture(scope="module")
def oracle_paths(orc):
    """(profile, B, L) -> (score, ids, sizes) of every candidate, computed once"""
    out = {}
    for B in bec.BLOCKS:
        for c in bec.candidates(B):
            p, seq = bec.window(c)
            score, xn, nd = orc.path(p.prof, bec.xt_of(orc, c.L), seq)
            assert np.isfinite(score)
            out[(c.pi, c.B, c.L)] = (score,) + orc.unzip(p.K, c.L, xn, nd)
    return out


def test_the_geometry_restated():
    """path_layout.block beside num_blocks: the blocks of a window tile its rows, the last ends at L, and lo is the last
    row of the block before"""
    for B in bec.BLOCKS + (0,):
        for L in range(1, 4 * max(B, 5) + 12):
            nb = num_blocks(L, B)
            blocks = [block(L, B, j) for j in range(nb)]
            assert blocks[0].lo == -1 and blocks[0].first == 0 and blocks[-1].last == L
            assert (nb == 1) == (B == 0 or L <= B + 5)
            for j in range(1, nb):
                assert blocks[j].lo == blocks[j - 1].last and blocks[j].first == blocks[j].lo + 1 <= blocks[j].last
                assert blocks[j].last - blocks[j].row_base < blocks[j].slots == B + 6


def test_the_table_holds_the_edges(oracle_paths):
    """coverage(): every crossing size, every landing offset in special, match and delete states, insert hand-overs at
    and below lo, and per class and B every residue of L mod 5 in several blocks and both sides of the first flip"""
    items = []
    for B in bec.BLOCKS:
        assert {L for L in bec.block_lengths(B)} >= {1, 4, 5, 6, B + 5, B + 6, 2 * B + 5, 2 * B + 6, 3 * B + 10}
        assert {num_blocks(L, B) for L in bec.block_lengths(B)} == {1, 2, 3, 4}
        for c in bec.cases(B):
            p = bec.profiles()[c.pi]
            items.append((p.cls, p.K, B, c.L) + oracle_paths[(c.pi, c.B, c.L)][1:])
    counts, missing = bec.coverage(items)
    print("crossing sizes", sorted(counts["sizes"].items()))
    for kind in bec.KINDS:
        print("hand-overs in", kind, "0..4 rows below lo:", [counts["landings"][(kind, o)] for o in range(5)])
    assert missing == []
    classes = {cls for (cls, _), _ in counts["per"]}
    assert classes >= {c for c, _ in bec.class_sizes()} and len(counts["per"]) == len(bec.profiles()) * len(bec.BLOCKS)
    assert {c.mode for B in bec.BLOCKS for c in bec.cases(B)} == {0, 1, 2, 3}


@pytest.mark.parametrize("G", bec.GROUPS)
def test_every_window_in_blocks(emul, orc, oracle_paths, G):
    """score bits and every step of every candidate, in a buffer of exactly N steps; no case is skipped.  A candidate
    that ties (the literal pass takes it) must be one the table leaves out: TIED is what the emulator finds, at most
    5 % of the candidates."""
    ties, total = set(), 0
    for B in bec.BLOCKS:
        for c in bec.candidates(B):
            total += 1
            score, ids, sizes = oracle_paths[(c.pi, c.B, c.L)]
            N = len(ids)
            n, got, buf, intact = emul.path(orc, c, G, N)
            assert bits(got) == bits(score) and intact, (c, G)
            if n == DCP_TB_TIE:
                ties.add((c.pi, c.B, c.L))
                continue
            assert n == N, (c, G, n, N)
            assert np.array_equal(buf & 0xFFFF, ids.astype(np.uint32)) and np.array_equal(buf >> 16, sizes.astype(np.uint32)), (c, G)
    print(f"G={G}: {total} candidates, {len(ties)} tied")
    assert ties == set(bec.TIED) and len(ties) <= bec.MAX_TIED * total


@pytest.mark.parametrize("G", bec.GROUPS)
def test_one_step_short_overflows(emul, orc, oracle_paths, G):
    """a buffer of N - 1 steps: DCP_TB_OVERFLOW, nothing written outside it.  Windows of one block, of two (one resume)
    and of four (the walk meets the limit in block 0, after three resumes: the count comes from DcpTraceState::n)"""
    resumes = set()
    for B in bec.BLOCKS:
        for c in bec.cases(B):
            if c.L not in (6, B + 6, 3 * B + 8) or bec.profiles()[c.pi].K > 4096:
                continue
            score, ids, sizes = oracle_paths[(c.pi, c.B, c.L)]
            N = len(ids)
            # where the walk stands when step N - 1 does not fit: the stage of the path's second state
            resumes.add(num_blocks(c.L, B) - 1 if int(np.cumsum(sizes)[1]) <= B + 5 else -1)
            n, got, buf, intact = emul.path(orc, c, G, N - 1)
            assert n == DCP_TB_OVERFLOW and intact and bits(got) == bits(score), (c, G, n)
            # the steps that fitted are the path's last N - 2, where they belong
            assert np.array_equal(buf[1:] & 0xFFFF, ids[2:].astype(np.uint32)), (c, G)
    assert {0, 1, 3} <= resumes
