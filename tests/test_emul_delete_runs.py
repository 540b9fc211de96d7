"""CPU: the lazy D->D turns of the cost kernels (dcp_lazy_turns_carry, deciphon_amd/csrc/viterbi_body.h) on the
64-lane emulator, with profiles whose best alignment deletes a planted run of 1 .. K - 2 positions
(tests/delete_run_cases.py).  A turn moves only the carry from lane to lane and D is written once at the end, so
what is checked here is that a value carried through r / Q lanes -- the turns taken without a vote, then the loop
behind the vote -- leaves the same bits as the reference's position-by-position recurrence: every single-wave
shape (1..8 and 10 positions per lane) at both ends of the profiles it serves, every shape of PackWave with
windows of different lengths in one pack, DD over the run 0.0, tiny and ordinary, plain and tie-rich tables."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from dcp_testlib import ROOT, bits, choose_qw, code_rows, pack_profile, reflib
from delete_run_cases import DD_KINDS, LAYOUT, LONG_RUN, PACK_SHAPES, SINGLE_WAVE, planted, run_lengths, single_wave_cases
from test_emul_kernels import Pack, _vp

EMUL_PACK_SHAPES = PACK_SHAPES + ((32, 6), (32, 8))  # the emulator also holds the two wide shapes


@pytest.fixture(scope="module")
def em():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "emul")], check=True)
    lib = C.CDLL(os.path.join(ROOT, "tests", "emul", "libdcp_emul.so"))
    yield lib
    # no emulated kernel read a row beyond its resource: nothing relies on what the buffer range rule returns there
    # (lane_ops_emul.h, em_row_range_zeros; DESIGN.md, "the two lane vocabularies")
    lib.emul_row_range_zeros.restype = C.c_long
    assert lib.emul_row_range_zeros() == 0


def votes(em):
    v = (C.c_long * 2)()
    em.emul_votes(v)
    return v[0], v[1]


def xtrans(orc, seq, quant):
    xt = orc.xtrans(max(len(seq) // 3, 1), True, False)
    return (np.round(xt / quant) * quant).astype(np.float32) if quant else xt


def on_shape(prof, Q):
    """the padded tables of the layout the (Q,1) kernel reads, with the kernel's own shape in the descriptor"""
    pool, pd = pack_profile(prof, *LAYOUT.get(Q, (Q, 1)))
    pd.Q, pd.W = Q, 1
    return pool, pd


def test_case_list_is_what_the_kernels_need():
    cases = single_wave_cases()
    assert {Q for Q, *_ in cases} == {1, 2, 3, 4, 5, 6, 7, 8, 10}
    assert {dd for *_, dd, _ in cases} == set(DD_KINDS) and any(q for *_, q in cases) and any(not q for *_, q in cases)
    for Q, K in SINGLE_WAVE:
        rs = run_lengths(K)
        assert rs[0] == 1 and rs[-1] == K - 2
    # a run of 4 * DCP_LAZY_POSITIONS positions crosses four or more lane boundaries in every shape (Q <= 6: at
    # least four, beyond that the loop behind the vote still has to take turns of its own)
    assert 3 * sum(r >= LONG_RUN for _, _, r, _, _ in cases) >= len(cases)


def test_single_wave_shapes(em, orc):
    ref = reflib()
    rng = np.random.default_rng(61)
    carried = {}
    for Q, K, r, dd, quant in single_wave_cases():
        prof, seq, a = planted(rng, K, r, dd, quant)
        xt = xtrans(orc, seq, quant)
        pool, pd = on_shape(prof, Q)
        xt16 = np.zeros(16, np.float32)
        xt16[:13] = xt
        out = np.zeros(2, np.float32)
        votes(em)
        assert em.emul_cost(_vp(pool), C.byref(pd), _vp(code_rows(seq)), len(seq), _vp(xt16), _vp(out)) == 0
        taken, again = votes(em)
        assert taken >= len(seq)
        want = orc.cost(prof, xt, seq)
        assert np.isfinite(want)
        assert bits(out[0]) == bits(orc.null(prof, xt, seq)), (Q, K, r, dd, quant, a)
        assert bits(out[1]) == bits(want), (Q, K, r, dd, quant, a)
        if ref is not None:
            ref.setup(prof)
            assert bits(out[0]) == bits(ref.null(xt, seq)) and bits(out[1]) == bits(ref.cost(xt, seq)), (Q, K, r, dd)
        if r >= LONG_RUN and dd != "ordinary":
            carried[Q] = carried.get(Q, 0) + again
    # nearly free runs of 24 positions and more: the turns taken without a vote cannot cover them in any shape
    assert all(carried.get(Q, 0) > 0 for Q in (1, 2, 3, 4, 5, 6, 7, 8, 10)), carried


def test_the_deleted_run_is_on_the_best_path(em, orc):
    """the planted run is what the scores above are made of: the oracle's path deletes exactly those positions"""
    rng = np.random.default_rng(62)
    for K, r in ((60, 37), (192, 150), (256, 24)):
        prof, seq, a = planted(rng, K, r, "tiny")
        xt = xtrans(orc, seq, None)
        _, xn, nd = orc.path(prof, xt, seq)
        ids, _ = orc.unzip(K, len(seq), xn, nd)
        deleted = sorted(int(s & 0x3FFF) for s in ids if (int(s) >> 14) == 2)
        assert deleted == list(range(a + 1, a + r + 1)), (K, r, a, deleted)


def test_stored_rows_replay_to_the_reference_trellis(em, orc):
    """the table-writing kernels share row(): D of every row, as stored, gives the oracle's trellis when the rows
    are replayed pass by pass (row_replay.h)"""
    rng = np.random.default_rng(63)
    for Q, K in SINGLE_WAVE:
        if Q in LAYOUT:
            continue  # the path pass runs the class's own shape
        for dd, quant in (("zero", None), ("tiny", 1.0)):
            r = max(r for r in run_lengths(K) if r <= max(K // 2, 1))
            prof, seq, a = planted(rng, K, r, dd, quant)
            L = len(seq)
            xt = xtrans(orc, seq, quant)
            pool, pd = on_shape(prof, Q)
            rows = code_rows(seq)
            xt16 = np.zeros(16, np.float32)
            xt16[:13] = xt
            out = np.zeros(2, np.float32)
            cells = np.full((L + 1) * 3 * pd.Kp, np.nan, np.float32)
            sp = np.full((L + 1) * 8, np.nan, np.float32)
            assert em.emul_cost_store(_vp(pool), C.byref(pd), _vp(rows), L, _vp(xt16), _vp(out), _vp(cells), _vp(sp)) == 0
            xn = np.full(L + 1, 0xFFFFFFFF, np.uint32)
            nd = np.full((L + 1) * K, 0xFFFF, np.uint16)
            assert em.emul_replay(_vp(pool), C.byref(pd), _vp(rows), L, _vp(xt16), _vp(cells), _vp(sp), _vp(xn), _vp(nd)) == 0
            score, xo, no = orc.path(prof, xt, seq)
            assert bits(out[1]) == bits(score), (Q, K, r, dd)
            assert np.array_equal(xn, xo) and np.array_equal(nd, no), (Q, K, r, dd, quant)


def test_pack_shapes_with_mixed_window_lengths(em, orc):
    """every group of a pack runs the same profile on a window of its own: the full planted read, the read cut
    short inside and behind the run, and a prefix that never reaches it -- lengths differ inside every pack, and a
    carry must stop at the separator lane of the next group"""
    ref = reflib()
    rng = np.random.default_rng(64)
    carried = {}
    for S, Q in EMUL_PACK_SHAPES:
        cap = (S - 1) * Q
        G = 64 // S
        for K in sorted({max(cap // 2 + 1, min(cap, 3)), cap}):
            if K < 3 or S * Q > 64 * choose_qw(K)[0]:  # the shape reads S * Q columns: never chosen for so short a row
                continue
            for r in run_lengths(K):
                for dd in DD_KINDS:
                    for quant in (None, 2.0):
                        prof, seq, a = planted(rng, K, r, dd, quant)
                        cuts = [len(seq), max(3 * a, 1), max(len(seq) - 3, 1), max(3 * a + 6, 1), len(seq) // 2 + 1]
                        seqs = [np.ascontiguousarray(seq[: min(cuts[g % len(cuts)], len(seq))]) for g in range(G)]
                        out, xt, again = run_pack(em, orc, prof, S, Q, seqs, quant)
                        for g, s in enumerate(seqs):
                            x = np.ascontiguousarray(xt[max(len(s) // 3, 1), :13])
                            assert bits(out[g, 0]) == bits(orc.null(prof, x, s)), (S, Q, K, r, dd, quant, g)
                            assert bits(out[g, 1]) == bits(orc.cost(prof, x, s)), (S, Q, K, r, dd, quant, g)
                            if ref is not None and g < 2:
                                ref.setup(prof)
                                assert bits(out[g, 1]) == bits(ref.cost(x, s)), (S, Q, K, r, dd, g)
                        if r >= LONG_RUN and dd != "ordinary":
                            carried[(S, Q)] = carried.get((S, Q), 0) + again
    # the shapes that hold 26 positions and more had runs of 24: their loops behind the vote ran
    assert all(n > 0 for n in carried.values()) and len(carried) >= 6, carried


def run_pack(em, orc, prof, S, Q, seqs, quant):
    """-> (float32 [n][2], xtrans table, votes that asked for one more turn)"""
    pool, pd = pack_profile(prof, *choose_qw(prof.K))
    rows, first = [], []
    for s in seqs:
        first.append(sum(len(r) for r in rows))
        rows.append(code_rows(s))
    rows = np.ascontiguousarray(np.concatenate(rows))
    smax = max(max(len(s) // 3, 1) for s in seqs)
    xt = np.zeros((smax + 1, 16), np.float32)
    for s in range(1, smax + 1):
        v = orc.xtrans(s, True, False)
        xt[s, :13] = (np.round(v / quant) * quant).astype(np.float32) if quant else v
    pk = Pack()
    pk.profile, pk.Lmax = 0, max(len(s) for s in seqs)
    out = np.full((len(seqs) + 3, 2), np.float32(-7.0), np.float32)
    for g, s in enumerate(seqs):
        pk.L[g], pk.xt_row[g], pk.out[g], pk.code_row[g] = len(s), max(len(s) // 3, 1), g, first[g]
    votes(em)
    assert em.emul_cost_pack(Q, S, _vp(pool), C.byref(pd), _vp(rows), len(rows), _vp(xt), C.byref(pk), _vp(out)) == 0
    assert np.all(out[len(seqs):] == np.float32(-7.0))
    again = votes(em)[1]
    if Q <= 4:  # the same windows with the short emission lengths' rows read from the LDS copy: the same bits
        out2 = np.full_like(out, np.float32(-7.0))
        assert em.emul_cost_pack_lds(Q, S, _vp(pool), C.byref(pd), _vp(rows), len(rows), _vp(xt), C.byref(pk), _vp(out2)) == 0
        assert np.array_equal(out.view(np.uint32), out2.view(np.uint32))
    return out[: len(seqs)], xt, again
