"""CPU: the two ends of the cost kernels' row loop on the 64-lane emulator (tests/row_loop_cases.py), bit for bit.

Short windows -- every length up to twelve rows and every residue of L mod 5 around larger lengths -- through every
single-wave shape and every pack shape against the oracle; finite junk at k = 0 of MM, MD, IM, DM, DD against the
same profile with +inf there, scores and paths; and packs whose groups end at different rows."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from dcp_testlib import ROOT, bits, choose_qw, code_rows, pack_profile, random_seq, synth_profile
from delete_run_cases import LAYOUT, SINGLE_WAVE
from row_loop_cases import K0_JUNK, WINDOW_LENGTHS, with_k0
from test_emul_kernels import PACK_SHAPES, _vp, run_pack, run_path


@pytest.fixture(scope="module")
def em():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "emul")], check=True)
    lib = C.CDLL(os.path.join(ROOT, "tests", "emul", "libdcp_emul.so"))
    yield lib
    # no emulated kernel read a row beyond its resource: nothing relies on what the buffer range rule returns there
    # (lane_ops_emul.h, em_row_range_zeros; DESIGN.md, "the two lane vocabularies")
    lib.emul_row_range_zeros.restype = C.c_long
    assert lib.emul_row_range_zeros() == 0


def cost_on_shape(em, prof, Q, xt, seq):
    """null and cost of one window through the (Q,1) kernel on the layout it reads"""
    pool, pd = pack_profile(prof, *LAYOUT.get(Q, (Q, 1)))
    pd.Q, pd.W = Q, 1
    xt16 = np.zeros(16, np.float32)
    xt16[:13] = xt
    out = np.zeros(2, np.float32)
    assert em.emul_cost(_vp(pool), C.byref(pd), _vp(code_rows(seq)), len(seq), _vp(xt16), _vp(out)) == 0
    return out


def pack_k(S, Q, rng):
    """a core size the pack shape (S, Q) is chosen for"""
    cap = (S - 1) * Q
    K = int(rng.integers(max(cap // 2, 1), cap + 1))
    return cap if S * Q > 64 * choose_qw(K)[0] else K


def test_short_windows_single_wave_shapes(em, orc):
    rng = np.random.default_rng(701)
    for Q, K in SINGLE_WAVE[1::2]:  # the upper end of every shape's range
        prof = synth_profile(rng, K, [None, 2.0][Q % 2])
        for L in WINDOW_LENGTHS:
            seq = random_seq(rng, L)
            xt = orc.xtrans(max(L // 3, 1), True, False)
            out = cost_on_shape(em, prof, Q, xt, seq)
            assert bits(out[0]) == bits(orc.null(prof, xt, seq)), (Q, K, L)
            assert bits(out[1]) == bits(orc.cost(prof, xt, seq)), (Q, K, L)


def test_short_windows_stored_rows_and_blocks(em, orc):
    """the table-writing and checkpoint kernels share the body: every row of a short window as stored, walked back
    by the traceback, for tables held whole and a block of five or ten rows at a time"""
    em.emul_path_blocks.restype = C.c_int
    rng = np.random.default_rng(702)
    for K in (17, 100, 192, 256, 384, 512):
        prof = synth_profile(rng, K)
        for L in WINDOW_LENGTHS[:22]:
            seq = random_seq(rng, L)
            xt = orc.xtrans(max(L // 3, 1), True, False)
            s_o, xo, no = orc.path(prof, xt, seq)
            ids, sizes = orc.unzip(K, L, xo, no)
            pool, pd = pack_profile(prof)
            xt16 = np.zeros(16, np.float32)
            xt16[:13] = xt
            for B in (0, 5, 10):
                cap = 2 * L + 2 * K + 64
                buf = np.zeros(cap, np.uint32)
                score = C.c_float(0)
                n = em.emul_path_blocks(_vp(pool), C.byref(pd), _vp(code_rows(seq)), L, _vp(xt16), B, 1 + B // 5, _vp(buf),
                                        C.c_long(cap), C.byref(score))
                assert bits(score.value) == bits(s_o), (K, L, B)
                if n == -2 or not np.isfinite(s_o):  # an exact tie the values cannot resolve: the literal pass takes it
                    continue
                w = buf[cap - n:]
                assert n > 0 and np.array_equal(w & 0xFFFF, ids.astype(np.uint32)), (K, L, B, n)
                assert np.array_equal(w >> 16, sizes.astype(np.uint32)), (K, L, B)


def test_short_windows_pack_shapes(em, orc):
    """all groups of a pack on windows of one length L (the loop's own end), full and partly filled packs"""
    rng = np.random.default_rng(703)
    for S, Q in PACK_SHAPES:
        prof = synth_profile(rng, pack_k(S, Q, rng), [None, 1.0][S // 8 % 2])
        G = 64 // S
        for L in WINDOW_LENGTHS[:17]:
            seqs = [random_seq(rng, L) for _ in range(G if L % 2 else max(G - 1, 1))]
            out, xt = run_pack(em, orc, prof, S, Q, seqs)
            for g, s in enumerate(seqs):
                x = np.ascontiguousarray(xt[max(L // 3, 1), :13])
                assert bits(out[g, 0]) == bits(orc.null(prof, x, s)), (S, Q, prof.K, L, g)
                assert bits(out[g, 1]) == bits(orc.cost(prof, x, s)), (S, Q, prof.K, L, g)


def test_windows_that_end_early_in_a_pack(em, orc):
    """groups of different lengths in one pack capture their results at their own last row: the longest window sits
    in any group, the others end one to Lmax - 1 rows earlier, in every residue of 5"""
    rng = np.random.default_rng(704)
    for S, Q in PACK_SHAPES:
        G = 64 // S
        prof = synth_profile(rng, pack_k(S, Q, rng))
        for Lmax in (2, 5, 6, 11, 23, 40):
            lens = [int(rng.integers(1, Lmax + 1)) for _ in range(G)]
            lens[int(rng.integers(0, G))] = Lmax
            if G > 1:
                lens[(lens.index(Lmax) + 1) % G] = max(Lmax - 1, 1)
            seqs = [random_seq(rng, n) for n in lens]
            out, xt = run_pack(em, orc, prof, S, Q, seqs)
            for g, s in enumerate(seqs):
                x = np.ascontiguousarray(xt[max(len(s) // 3, 1), :13])
                assert bits(out[g, 0]) == bits(orc.null(prof, x, s)), (S, Q, prof.K, lens, g)
                assert bits(out[g, 1]) == bits(orc.cost(prof, x, s)), (S, Q, prof.K, lens, g)


def test_junk_at_position_zero_single_wave_shapes(em, orc):
    """what a caller's tables hold at k = 0 of MM, MD, IM, DM, DD reaches no score and no path"""
    em.emul_path_blocks.restype = C.c_int
    rng = np.random.default_rng(705)
    for Q, K in SINGLE_WAVE:
        base = synth_profile(rng, K, [None, 1.0][K % 2])
        seq = random_seq(rng, int(rng.integers(6, 30)))
        L = len(seq)
        xt = orc.xtrans(max(L // 3, 1), True, False)
        clean = with_k0(base, None)
        want = cost_on_shape(em, clean, Q, xt, seq)
        assert bits(want[0]) == bits(orc.null(clean, xt, seq)) and bits(want[1]) == bits(orc.cost(clean, xt, seq)), (Q, K)
        walks = []
        for junk in (None,) + K0_JUNK:
            prof = with_k0(base, junk)
            got = cost_on_shape(em, prof, Q, xt, seq)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (Q, K, junk)
            if Q in LAYOUT:
                continue  # the path pass runs the class's own shape
            pool, pd = pack_profile(prof)
            xt16 = np.zeros(16, np.float32)
            xt16[:13] = xt
            cap = 2 * L + 2 * K + 64
            buf = np.zeros(cap, np.uint32)
            score = C.c_float(0)
            n = em.emul_path_blocks(_vp(pool), C.byref(pd), _vp(code_rows(seq)), L, _vp(xt16), 10, 2, _vp(buf), C.c_long(cap),
                                    C.byref(score))
            walks.append((bits(score.value), n, buf[cap - n:].tobytes() if n > 0 else b""))
            if K <= 256:  # the literal pass: every trellis word
                s, xn, nd = run_path(em, prof, xt, seq)
                s_o, xo, no = orc.path(clean, xt, seq)
                assert bits(s) == bits(s_o) and np.array_equal(xn, xo) and np.array_equal(nd, no), (Q, K, junk)
        assert all(w == walks[0] for w in walks), (Q, K)


def test_junk_at_position_zero_pack_shapes(em, orc):
    rng = np.random.default_rng(706)
    for S, Q in PACK_SHAPES:
        base = synth_profile(rng, pack_k(S, Q, rng))
        seqs = [random_seq(rng, int(rng.integers(1, 30))) for _ in range(64 // S)]
        want, xt = run_pack(em, orc, with_k0(base, None), S, Q, seqs)
        for g, s in enumerate(seqs):
            x = np.ascontiguousarray(xt[max(len(s) // 3, 1), :13])
            assert bits(want[g, 1]) == bits(orc.cost(with_k0(base, None), x, s)), (S, Q, g)
        for junk in K0_JUNK:
            got, _ = run_pack(em, orc, with_k0(base, junk), S, Q, seqs)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (S, Q, junk)
