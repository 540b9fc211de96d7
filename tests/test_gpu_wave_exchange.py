"""GPU: the cases of tests/test_emul_wave_exchange.py -- short-anchor planted runs on every multi-wave cost shape and
the strip class, at both ends of the profiles each serves (tests/delete_run_cases.py) -- through Engine.cost and
Engine.path, bit for bit against the oracle.  The profiles come from the same seeds in the same order, so what the
emulator test asserts about them holds here: per shape the sweep of the delete cost has windows whose rows all keep
the one-barrier exchange, windows whose rows all leave it and windows with both (MIXED_AT names one), and with the
late entry blocked the best path deletes a whole wavefront (strip).  The LDS flags and barriers of the second protocol
(put_last / get_shift / put_any / get_any, lane_ops_gpu.h) exist on the GPU alone.  A subset per shape goes through
the path pass as the engine runs it by default, in blocks of 15 rows (dcp_cost_ckpt_kernel, dcp_cost_store_kernel,
dcp_path_blocks_kernel share CostWave::row) and pass by pass (PathWave)."""
import numpy as np
import pytest

from dcp_testlib import bits
from delete_run_cases import (ANCHOR, CANCEL_QUANT, CANCEL_SHAPES, MIXED_AT, SWEEP, WINDOW, cancelling_run, short_anchor,
                              wave_cases, wave_shapes)

pytestmark = pytest.mark.gpu

SEED = 9000  # + K, as tests/test_emul_wave_exchange.py
PATH_ENV = ("DECIPHON_HIP_PATH", "DECIPHON_HIP_CKPT_ROWS", "DECIPHON_HIP_PATH_GROUP", "DECIPHON_HIP_PATH_FUSED",
            "DECIPHON_HIP_PATH_BUDGET_MB", "DECIPHON_HIP_PATH_STRICT")
MODES = {"default": {},
         "blocks of 15 rows": {"DECIPHON_HIP_CKPT_ROWS": "16"},
         "blocks, one launch per window": {"DECIPHON_HIP_CKPT_ROWS": "16", "DECIPHON_HIP_PATH_GROUP": "1"},
         "blocks, a launch per block": {"DECIPHON_HIP_CKPT_ROWS": "16", "DECIPHON_HIP_PATH_GROUP": "1",
                                        "DECIPHON_HIP_PATH_FUSED": "0"},
         "pass by pass": {"DECIPHON_HIP_PATH": "literal"}}


def xtrans(orc, quant):
    xt = orc.xtrans(WINDOW // 3, True, False)
    return (np.round(xt / quant) * quant).astype(np.float32) if quant else xt


def load(engine, orc, profs, reads, quant):
    engine.clear_profiles()
    for p in profs:
        engine.add_profile(p.K, p.trans, p.match, p.null, p.bg)
    engine.commit()
    engine.set_sequences(reads)
    engine.set_mode(True, False)
    table = np.zeros((0, 13), np.float32)
    if quant:
        table = np.zeros((WINDOW // 3 + 2, 13), np.float32)
        for s in range(1, len(table)):
            table[s] = (np.round(orc.xtrans(s, True, False) / quant) * quant).astype(np.float32)
    engine.set_xtrans_table(table)


def set_mode(monkeypatch, env):
    for name in PATH_ENV:
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)


def check_path(orc, res, prof, seq, xt, what, trellis=True):
    score, xo, no = orc.path(prof, xt, seq)
    ids, sizes = orc.unzip(prof.K, len(seq), xo, no)
    assert bits(res["score"]) == bits(score), what
    assert np.array_equal(res["state_ids"], ids) and np.array_equal(res["seqsizes"], sizes), what
    if trellis:
        assert np.array_equal(res["xnodes"], xo) and np.array_equal(res["nodes"], no), what
        assert bits(res["literal_score"]) == bits(score), what
        assert np.array_equal(res["literal_state_ids"], ids) and np.array_equal(res["literal_seqsizes"], sizes), what


@pytest.mark.parametrize("Q,W,K,span,brief", wave_shapes())
def test_multi_wave_shapes(engine, orc, monkeypatch, Q, W, K, span, brief):
    rng = np.random.default_rng(SEED + K)
    cases = wave_cases(Q, W, K, span, brief)
    made = [short_anchor(rng, K, a, r, dd, entry, everywhere, quant) for _, a, r, dd, entry, everywhere, quant in cases]
    assert len(made) <= 50
    set_mode(monkeypatch, {})
    try:
        for quant in sorted({c[6] for c in cases}, key=lambda q: q or 0.0):
            idx = [i for i, c in enumerate(cases) if c[6] == quant]
            profs, reads = [made[i][0] for i in idx], [made[i][1] for i in idx]
            load(engine, orc, profs, reads, quant)
            wins = [(j, j, 0, WINDOW) for j in range(len(idx))]
            xt = xtrans(orc, quant)
            nul, alt = engine.cost(wins)  # one call over all windows of the class
            for j, i in enumerate(idx):
                assert bits(nul[j]) == bits(orc.null(profs[j], xt, reads[j])), (K, cases[i])
                assert bits(alt[j]) == bits(orc.cost(profs[j], xt, reads[j])), (K, cases[i])
            # the path pass: a free whole-wavefront run with the entry blocked, one window of the sweep with rows on
            # either protocol, a tie-rich one
            sel = [j for j, i in enumerate(idx) if cases[i][0] == "whole" and cases[i][3:5] == ("zero", "blocked")
                   or (cases[i][4] == "open" and not quant and K in MIXED_AT and cases[i][3] == SWEEP[MIXED_AT[K]])]
            assert len(sel) == (0 if quant and quant != 1.0 else 1 if quant or brief else 2), (K, quant, sel)
            if not sel:
                continue
            for mode, env in MODES.items():
                if span and mode not in ("default", "blocks of 15 rows"):
                    continue  # the strip class in blocks and under a budget: test_strips_under_a_budget
                set_mode(monkeypatch, env)
                res = engine.path([wins[j] for j in sel], trellis=True)
                for j, p in zip(sel, res):
                    check_path(orc, p, profs[j], reads[j], xt, (K, mode, cases[idx[j]]))
            set_mode(monkeypatch, {})
    finally:
        engine.set_xtrans_table(np.zeros((0, 13), np.float32))


@pytest.mark.parametrize("K", [6144, 16383])
def test_strips_under_a_budget(orc, monkeypatch, K):
    """one whole strip deleted, the window's table (48 rows of 3 Kp floats) above the budget: taken from checkpoints in
    three blocks, fast pass and replayed trellis"""
    import deciphon_amd

    from delete_run_cases import STRIP, STRIP_Q, wave_geometries

    rng = np.random.default_rng(SEED + 11 * K)
    a, r = wave_geometries(K, 64 * STRIP_Q, STRIP)["whole strip"]
    prof, seq = short_anchor(rng, K, a, r, "zero")
    Kp = (K + STRIP - 1) // STRIP * STRIP
    table = (WINDOW + 1) * (8 + 3 * Kp) * 4
    budget = table * 3 // 4 >> 20
    assert (budget << 20) < table
    set_mode(monkeypatch, {"DECIPHON_HIP_CKPT_ROWS": "16", "DECIPHON_HIP_PATH_GROUP": "1",
                           "DECIPHON_HIP_PATH_BUDGET_MB": str(budget)})
    xt = xtrans(orc, None)
    with deciphon_amd.Engine(0) as eng:
        eng.add_profile(prof.K, prof.trans, prof.match, prof.null, prof.bg)
        eng.commit()
        eng.set_sequences([seq])
        eng.set_mode(True, False)
        win = [(0, 0, 0, WINDOW)]
        nul, alt = eng.cost(win)
        assert bits(alt[0]) == bits(orc.cost(prof, xt, seq)) and bits(nul[0]) == bits(orc.null(prof, xt, seq))
        p = eng.path(win, trellis=False)[0]
        assert eng.path_blocked == 1 and eng.path_redone == 0
        check_path(orc, p, prof, seq, xt, (K, "fast pass in blocks"), trellis=False)
        check_path(orc, eng.path(win, trellis=True)[0], prof, seq, xt, (K, "trellis in blocks"))


def test_a_whole_wave_run_at_640_positions(engine, orc, monkeypatch):
    """K = 640: the cost pass is the narrow (10,1) kernel, the path pass writes its tables with the (6,2) kernels"""
    K, per = 640, 384
    rng = np.random.default_rng(SEED + K)
    made = [short_anchor(rng, K, per + da, K - ANCHOR - per - da, dd) for da, dd in ((0, "zero"), (-1, "tiny"), (1, "zero"))]
    profs, reads = [m[0] for m in made], [m[1] for m in made]
    set_mode(monkeypatch, {})
    load(engine, orc, profs, reads, None)
    wins = [(j, j, 0, WINDOW) for j in range(len(made))]
    xt = xtrans(orc, None)
    nul, alt = engine.cost(wins)
    for j in range(len(made)):
        assert bits(alt[j]) == bits(orc.cost(profs[j], xt, reads[j])) and bits(nul[j]) == bits(orc.null(profs[j], xt, reads[j]))
    for mode in ("default", "blocks of 15 rows", "blocks, a launch per block"):
        set_mode(monkeypatch, MODES[mode])
        for j, p in enumerate(engine.path(wins, trellis=True)):
            check_path(orc, p, profs[j], reads[j], xt, (K, mode, j))
    set_mode(monkeypatch, {})


@pytest.mark.parametrize("Q,W,K,span", CANCEL_SHAPES)
def test_a_run_that_cancels_what_entered_it(engine, orc, monkeypatch, Q, W, K, span):
    """negative match costs, E + tdd(1) = 2.0006 of |E| = 996 and tdd(1) = 998: the case that a margin relative to
    E + tdd(w) got wrong (tests/test_emul_wave_exchange.py has the figures) -- cost and path, whole tables and blocks"""
    rng = np.random.default_rng(4000 + K)
    xt = xtrans(orc, CANCEL_QUANT)
    prof, seq, f = cancelling_run(rng, Q, K, xt)
    assert f["chain"] < f["own"] <= f["relative"] and f["own"] > f["absolute"]
    set_mode(monkeypatch, {})
    try:
        load(engine, orc, [prof], [seq], CANCEL_QUANT)
        win = [(0, 0, 0, WINDOW)]
        nul, alt = engine.cost(win)
        assert bits(nul[0]) == bits(orc.null(prof, xt, seq))
        assert bits(alt[0]) == bits(orc.cost(prof, xt, seq)), (K, alt[0], orc.cost(prof, xt, seq))
        for mode in ("default", "blocks of 15 rows"):
            set_mode(monkeypatch, MODES[mode])
            check_path(orc, engine.path(win, trellis=True)[0], prof, seq, xt, (K, mode))
        set_mode(monkeypatch, {})
    finally:
        engine.set_xtrans_table(np.zeros((0, 13), np.float32))
