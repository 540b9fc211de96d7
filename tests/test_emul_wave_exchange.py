"""CPU: the exchange between the wavefronts of a row (CostWave<Q, W>, W > 1, and StripWave, deciphon_amd/csrc/
viterbi_body.h) on the emulator, with short-anchor planted runs (tests/delete_run_cases.py: short_anchor, wave_cases).
A row takes one barrier when E + tdd(w) >= D_last(w) proves the D every wavefront published final, and the
exchange-until-stable protocol otherwise; the GPU cannot say which one a row took, the emulator can
(emul_fallback_rows).  So this file does two things for tests/test_gpu_wave_exchange.py, which runs the same cases from
the same seeds: it checks every case bit for bit against the oracle here, and it ASSERTS what makes the GPU run mean
something -- per shape the sweep of the delete cost has cases with no row, with every row and with some rows on the
second protocol, and with the late entry blocked the best path deletes every position of a whole wavefront (strip),
which is the hazard the one-barrier shortcut guards against.  The emulator adds the DD of a wavefront in the order
the GPU does (lane_ops_emul.h, wave_tdd), so the same rows fall back here and there."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from dcp_testlib import ROOT, bits, choose_qw, code_rows, pack_profile, reflib
from delete_run_cases import (ANCHOR, CANCEL_QUANT, CANCEL_SHAPES, MIXED_AT, MULTI_WAVE, STRIP, STRIP_KS, STRIP_Q, STRIP_W,
                              SWEEP, WINDOW, cancelling_run, short_anchor, wave_cases, wave_geometries, wave_shapes)
from test_emul_kernels import _vp

SEED = 9000  # + K: tests/test_gpu_wave_exchange.py builds the same profiles


@pytest.fixture(scope="module")
def em():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "emul")], check=True)
    lib = C.CDLL(os.path.join(ROOT, "tests", "emul", "libdcp_emul.so"))
    lib.emul_fallback_rows.restype = C.c_long
    yield lib
    # no emulated kernel read a row beyond its resource: nothing relies on what the buffer range rule returns there
    # (lane_ops_emul.h, em_row_range_zeros; DESIGN.md, "the two lane vocabularies")
    lib.emul_row_range_zeros.restype = C.c_long
    assert lib.emul_row_range_zeros() == 0


def xtrans(orc, seq, quant):
    xt = orc.xtrans(max(len(seq) // 3, 1), True, False)
    return (np.round(xt / quant) * quant).astype(np.float32) if quant else xt


def xt16(xt):
    out = np.zeros(16, np.float32)
    out[:13] = xt
    return out


def strips_of(K, span):
    return (K + span - 1) // span if span else 1


def cost(em, prof, seq, xt, Q, W, strips, table=False):
    """-> (out[2], rows that left the one-barrier protocol[, cells, sp, pd, pool])"""
    pool, pd = pack_profile(prof, Q, W, strips)
    L = len(seq)
    out = np.zeros(2, np.float32)
    cells = np.full((L + 1) * 3 * pd.Kp, np.nan, np.float32) if table else None
    sp = np.full((L + 1) * 8, np.nan, np.float32) if table else None
    em.emul_fallback_rows()
    if strips > 1:
        ring = np.full(10 * pd.Kp, np.nan, np.float32)
        rc = em.emul_strip_cost(_vp(pool), C.byref(pd), _vp(code_rows(seq)), L, _vp(xt16(xt)), _vp(out), _vp(ring),
                                _vp(cells) if table else None, _vp(sp) if table else None)
    elif table:
        rc = em.emul_cost_store(_vp(pool), C.byref(pd), _vp(code_rows(seq)), L, _vp(xt16(xt)), _vp(out), _vp(cells), _vp(sp))
    else:
        rc = em.emul_cost(_vp(pool), C.byref(pd), _vp(code_rows(seq)), L, _vp(xt16(xt)), _vp(out))
    assert rc == 0
    fell = em.emul_fallback_rows()
    return (out, fell, cells, sp, pd, pool) if table else (out, fell)


def deleted_positions(orc, K, L, xn, nd):
    ids, _ = orc.unzip(K, L, xn, nd)
    return sorted(int(s & 0x3FFF) - 1 for s in ids if (int(s) >> 14) == 2)  # 0-based


def holds_aligned(deleted, per, K):
    """does the path delete every position of one whole, aligned block of `per` positions?"""
    d = set(deleted)
    return any(all(k in d for k in range(s, s + per)) for s in range(0, K - per + 1, per))


def on_path_shape(i, entry, dd, quant):
    """which cases of a profile beyond 1024 positions also go through the emulated path pass, which takes most of this
    file's time and has no shortcut of its own (PathWave exchanges pass by pass): every other blocked run, the
    tie-rich ones, and the sweep where the decision flips"""
    if quant or entry == "blocked":
        return bool(quant) or i % 2 == 0
    return not isinstance(dd, str) and SWEEP[8] <= dd <= SWEEP[15] and SWEEP.index(dd) % 2 == 0


def test_case_list_is_what_the_exchange_needs():
    """pins the list: every (Q, W) of classes 6..10 and the strip class at both ends of the profiles it serves, the
    nine runs around one whole wavefront, the strip boundaries, and a sweep of 16 values and more"""
    assert {(Q, W) for Q, W, _ in MULTI_WAVE} == {(6, 2), (4, 4), (6, 4), (8, 4), (8, 8)}
    assert [K for _, _, K in MULTI_WAVE] == [641, 768, 769, 1024, 1025, 1536, 1537, 2048, 2049, 4096]
    for Q, W, K in MULTI_WAVE:
        assert choose_qw(K) == (Q, W) and (K == 641 or choose_qw(K - 1) != (Q, W) or K == 64 * Q * W)
    assert (STRIP_Q, STRIP_W, STRIP) == (4, 8, 2048) and STRIP_KS == (4097, 6144, 16383)
    assert len(SWEEP) >= 16 and SWEEP[0] == np.float32(1e-3) and SWEEP[-1] == 1.0
    assert all(b > a for a, b in zip(SWEEP, SWEEP[1:]))
    for Q, W, K, span, brief in wave_shapes():
        per = 64 * Q
        geo = wave_geometries(K, per, span)
        nine = {n: g for n, g in geo.items() if n.startswith("whole") and n != "whole strip"}
        assert len(nine) == 9 and len(set(nine.values())) == 9
        if W > 2:  # exactly wavefront 1, and off by one at either end
            assert {g for g in nine.values()} == {(per + da, per + dr) for da in (-1, 0, 1) for dr in (-1, 0, 1)}
        else:  # no room behind wavefront 1: around its first position, up to the last position a run can end at
            assert {a for a, _ in nine.values()} == {per - 1, per, per + 1}
            assert {a + r for a, r in nine.values()} == {K - ANCHOR - 2, K - ANCHOR - 1, K - ANCHOR}
        assert geo["inside"][1] == 24 and geo["inside"][0] // per == (geo["inside"][0] + 23) // per
        a, r = geo["mid to mid"]
        assert a % per == per // 2 and r == per
        a, r = geo["to the end"]
        assert a + r - 1 == K - ANCHOR - 1
        a, r = geo["mid of wave 0 into the last wave"]
        assert a < per and (a + r - 1) // per == (min(K, span or K) - 1) // per or a + r == K - ANCHOR
        if span:
            assert [geo[f"across the strip boundary, from {b}"][0] + 40 for b in (2047, 2048, 2049)] == [2047, 2048, 2049]
            assert ("whole strip" in geo) == (K >= 2 * span + ANCHOR)
            if "whole strip" in geo:
                assert geo["whole strip"] == (span, span)
        cases = wave_cases(Q, W, K, span, brief)
        assert {c[0] for c in cases if c[4] == "blocked"} >= (set(geo) if not brief else {"whole", "to the end"})
        if not brief:
            assert [c[3] for c in cases if c[4] == "open" and not isinstance(c[3], str) and not c[6]] == list(SWEEP)
            assert {c[3] for c in cases if isinstance(c[3], str)} == {"zero", "tiny", "ordinary"}
            assert sum(1 for c in cases if c[6]) == 3


@pytest.mark.parametrize("Q,W,K,span,brief", wave_shapes())
def test_multi_wave_shapes(em, orc, Q, W, K, span, brief):
    """cost (null and alt) of every case, and -- below the strip class -- every word of the path pass's trellis on the
    shape it runs ((3, 2W) / (4, 2W)), against the oracle and the reference's own code where it is built"""
    ref = reflib()
    rng = np.random.default_rng(SEED + K)
    strips = strips_of(K, span)
    sweep, whole = [], []
    for i, (name, a, r, dd, entry, everywhere, quant) in enumerate(wave_cases(Q, W, K, span, brief)):
        what = (K, name, a, r, dd, entry, everywhere, quant)
        prof, seq = short_anchor(rng, K, a, r, dd, entry, everywhere, quant)
        assert len(seq) == WINDOW
        xt = xtrans(orc, seq, quant)
        out, fell = cost(em, prof, seq, xt, Q, W, strips)
        score, xo, no = orc.path(prof, xt, seq)
        assert np.isfinite(score)
        assert bits(out[0]) == bits(orc.null(prof, xt, seq)), what
        assert bits(out[1]) == bits(orc.cost(prof, xt, seq)) == bits(score), what
        if ref is not None and (K <= 1024 or i % 3 == 0):  # (beyond 1024 positions: every third case)
            ref.setup(prof)
            assert bits(out[0]) == bits(ref.null(xt, seq)) and bits(out[1]) == bits(ref.cost(xt, seq)), what
        if not span and (K <= 1024 or on_path_shape(i, entry, dd, quant)):
            pool, pd = pack_profile(prof, *choose_qw(K, path=True))
            xn = np.zeros(WINDOW + 1, np.uint32)
            nd = np.zeros((WINDOW + 1) * K, np.uint16)
            sc = C.c_float(0)
            assert em.emul_path(_vp(pool), C.byref(pd), _vp(code_rows(seq)), WINDOW, _vp(xt16(xt)), _vp(xn), _vp(nd), C.byref(sc)) == 0
            assert bits(sc.value) == bits(score), what
            assert np.array_equal(xn, xo) and np.array_equal(nd, no), what
        if entry == "open" and not isinstance(dd, str) and not quant:
            sweep.append(fell)
        if entry == "blocked" and dd in ("zero", "tiny") and not quant:
            deleted = deleted_positions(orc, K, WINDOW, xo, no)
            assert set(range(a, a + r)) <= set(deleted), what  # the run is on the best path
            whole.append((name, holds_aligned(deleted, 64 * Q, K), bool(span) and holds_aligned(deleted, span, K)))
    rows = WINDOW  # (strips: the counter takes every exchange, one per row and strip, and the sweep's run lies in the first)
    if not brief:
        # both protocols, and the decision inside one window: what the GPU run of the same cases then covers
        assert len(sweep) == len(SWEEP)
        assert any(f == 0 for f in sweep), (K, sweep)
        assert any(f >= rows for f in sweep), (K, sweep)
        assert any(0 < f < rows for f in sweep), (K, sweep)
        assert 0 < sweep[MIXED_AT[K]] < rows, (K, sweep)  # the one that the GPU test also takes a path of
    # the best path deletes a whole aligned wavefront -- where one fits between the anchors: with two wavefronts
    # wavefront 0 would need a run from position 0 and wavefront 1 one to position K - 1, so there the run covers all
    # of wavefront 1 but the closing anchor (`to the end`, asserted above to be on the path)
    if W > 2:
        assert any(w for n, w, _ in whole if n == "whole"), (K, whole)
    else:
        assert "to the end" in {n for n, _, _ in whole}
    if span and K >= 2 * span + ANCHOR:
        assert any(s for n, _, s in whole if n == "whole strip"), (K, whole)


@pytest.mark.parametrize("Q,W,K,span,brief", wave_shapes())
def test_stored_rows_replay_to_the_reference_trellis(em, orc, Q, W, K, span, brief):
    """the table-writing kernels share row(): M, I, D of every row as stored give the oracle's trellis when replayed
    (row_replay.h) -- one blocked and one open case per shape, the open one with some rows on each protocol where the
    sweep has such a value"""
    rng = np.random.default_rng(SEED + 7 * K)
    strips = strips_of(K, span)
    geo = wave_geometries(K, 64 * Q, span)
    name = "to the end" if W == 2 else "whole strip" if "whole strip" in geo else "whole"
    for dd, entry, everywhere in (("zero", "blocked", False), (SWEEP[12], "open", W == 2)):
        a, r = geo[name]
        prof, seq = short_anchor(rng, K, a, r, dd, entry, everywhere)
        xt = xtrans(orc, seq, None)
        out, fell, cells, sp, pd, pool = cost(em, prof, seq, xt, Q, W, strips, table=True)
        xn = np.full(WINDOW + 1, 0xFFFFFFFF, np.uint32)
        nd = np.full((WINDOW + 1) * K, 0xFFFF, np.uint16)
        assert em.emul_replay(_vp(pool), C.byref(pd), _vp(code_rows(seq)), WINDOW, _vp(xt16(xt)), _vp(cells), _vp(sp), _vp(xn), _vp(nd)) == 0
        score, xo, no = orc.path(prof, xt, seq)
        assert bits(out[1]) == bits(score), (K, dd, entry)
        assert np.array_equal(xn, xo) and np.array_equal(nd, no), (K, dd, entry)
        if entry == "blocked" and W > 2:  # (two wavefronts: nothing reads what the last one published)
            assert fell > 0, (K, fell)


def cancel_xt(orc):
    xt = orc.xtrans(2 * ANCHOR, True, False)
    return (np.round(xt / CANCEL_QUANT) * CANCEL_QUANT).astype(np.float32)


@pytest.mark.parametrize("Q,W,K,span", CANCEL_SHAPES)
def test_a_run_that_cancels_what_entered_it(em, orc, Q, W, K, span):
    """Negative match costs (the engine accepts them; only MD and DD must be non-negative): E = -996.25 enters
    wavefront 1 and 64 * Q - 1 delete steps of about +1000 / (64 * Q) each bring it to 1.99x, every step rounding down,
    3e-3 to 8e-3 below s = E + tdd(1) = 2.0006 (delete_run_cases.cancelling_run).  A margin of 1e-4 * |s| = 2e-4 does
    not cover that: with the wavefront's own D placed between the chain and s * 0.9999 the row kept its one barrier,
    the next wavefront started from the stale D, and the score came out -1993.5005 where the reference has -1993.5044
    ((4,4), K = 1024; (8,4), K = 2048: -1993.5001 / -1993.5079) -- this test failed on every shape.  The margin is now
    1e-4 * (|E| + tdd(w)), which bounds what 511 additions of magnitudes up to |E| + tdd(w) can round (511 * 2^-24 =
    3.1e-5 of it, viterbi_body.h); with non-negative costs it is the margin it was.  Tried before and never a mismatch:
    the blind sweeps of an uneven DD under anchors of -125, which do not put E + tdd next to D_last (about 10 000
    runs at K = 1024)."""
    rng = np.random.default_rng(4000 + K)
    xt = cancel_xt(orc)
    prof, seq, f = cancelling_run(rng, Q, K, xt)
    l, a, r = f["l"], f["a"], f["r"]
    out, fell, cells, sp, pd, pool = cost(em, prof, seq, xt, Q, W, strips_of(K, span), table=True)
    cells = cells.reshape(WINDOW + 1, 3, pd.Kp)
    # the case is what its builder says: E of row l stands at wavefront 0's last position, the chain through all of
    # wavefront 1 beats the wavefront's own D by less than the chain has rounded, and a margin relative to s misses it
    assert bits(cells[l, 0, a - 1]) == bits(f["E"]) == bits(np.nanmin(cells[l, 0, :K]))
    assert cells[l, 0, a + r - 2] == np.float32(-10.0)
    assert f["chain"] < f["own"] <= f["relative"] and f["own"] - f["chain"] < f["exact"] - f["chain"]
    assert f["s"] * np.float32(1 + 1e-4) >= f["own"] > f["absolute"] + np.float32(1e-3)
    assert abs(float(f["s"])) < 3 and abs(float(f["E"])) > 900 and float(f["tdd"]) > 900
    assert bits(cells[l, 2, a + r - 1]) == bits(f["chain"])  # D as stored: the chain is what the reference has there
    assert fell >= 1
    score, xo, no = orc.path(prof, xt, seq)
    assert bits(out[0]) == bits(orc.null(prof, xt, seq))
    assert bits(out[1]) == bits(orc.cost(prof, xt, seq)) == bits(score), (K, out[1], score)
    assert set(range(a, a + r)) <= set(deleted_positions(orc, K, WINDOW, xo, no))  # the score is made of that chain
    ref = reflib()
    if ref is not None:
        ref.setup(prof)
        assert bits(out[1]) == bits(ref.cost(xt, seq))
    xn = np.full(WINDOW + 1, 0xFFFFFFFF, np.uint32)
    nd = np.full((WINDOW + 1) * K, 0xFFFF, np.uint16)
    cells = np.ascontiguousarray(cells.reshape(-1))
    assert em.emul_replay(_vp(pool), C.byref(pd), _vp(code_rows(seq)), WINDOW, _vp(xt16(xt)), _vp(cells), _vp(sp), _vp(xn), _vp(nd)) == 0
    assert np.array_equal(xn, xo) and np.array_equal(nd, no)
