"""GPU: the windows of tests/block_edge_cases.py -- the table that tests/test_emul_block_edges.py runs on the wave
emulator, same seeds -- through Engine.path under DECIPHON_HIP_CKPT_ROWS = 5, 10, 20 in every launch form of the fast
pass: all windows of all classes of a B in one request, score bits and every step against the oracle, and no window
redone (the table holds no ties: a redo is a traceback that gave up where the emulator's did not).  Then the literal
pass of one window per class and residue of L mod 5, every trellis word against the oracle.

The strip class (K > 4096) keeps a window's whole table where the budget holds it, and a table of 70 rows is 5 MB.  So
the forms that set DECIPHON_HIP_PATH_GROUP also set DECIPHON_HIP_PATH_BUDGET_MB=1, the smallest there is: the strip
windows of 14 rows or more then go in blocks like every other class (path_blocked says how many), the shorter ones --
B = 5: the flip at 10 | 11 rows among them -- keep their table.  The engine has its arena reserved beforehand, so the
request is still placed as one slice and the kernels of the classes run side by side."""
import time

import numpy as np
import pytest

import block_edge_cases as bec
from dcp_testlib import bits
from path_layout import MB, literal_bytes, num_blocks, table_bytes

pytestmark = pytest.mark.gpu

ENV = ("DECIPHON_HIP_CKPT_ROWS", "DECIPHON_HIP_PATH_GROUP", "DECIPHON_HIP_PATH_FUSED", "DECIPHON_HIP_PATH",
       "DECIPHON_HIP_PATH_BUDGET_MB", "DECIPHON_HIP_PATH_STRICT", "DECIPHON_HIP_UNZIP_CAP")
SMALL = {"DECIPHON_HIP_PATH_BUDGET_MB": "1"}
FORMS = (("default", {}),
         ("a block per round, one launch", dict(SMALL, DECIPHON_HIP_PATH_GROUP="1")),
         ("a launch per block and phase", dict(SMALL, DECIPHON_HIP_PATH_GROUP="1", DECIPHON_HIP_PATH_FUSED="0")),
         ("three blocks side by side", dict(SMALL, DECIPHON_HIP_PATH_GROUP="3")))


def set_form(monkeypatch, B, env):
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("DECIPHON_HIP_CKPT_ROWS", str(B))
    for name, value in env.items():
        monkeypatch.setenv(name, value)


def gpu_profiles():
    """-> (profile index of the table -> index in the engine, [Prof]) without the emulator's own strip shapes"""
    keep = [pi for pi, p in enumerate(bec.profiles()) if not p.emul]
    return {pi: i for i, pi in enumerate(keep)}, [bec.profiles()[pi] for pi in keep]


def load_engine(orc, reserve=0):
    """a fresh Engine with the table's profiles, their reads and the special transitions of all four modes"""
    import deciphon_amd

    eng = deciphon_amd.Engine(0)
    _, profs = gpu_profiles()
    for p in profs:
        eng.add_profile(p.K, p.prof.trans, p.prof.match, p.prof.null, p.prof.bg)
    eng.commit()
    eng.set_sequences([p.read for p in profs])
    eng.set_mode(True, False)
    eng.set_xtrans_table(bec.xt_table(orc))
    if reserve:
        eng.path_reserve(reserve)
    return eng


def windows_of(cases):
    index, _ = gpu_profiles()
    return [(index[c.pi], index[c.pi], c.a, c.a + c.L) for c in cases]


_oracle = {}


def oracle_of(orc, c, trellis=False):
    """-> (score, ids, sizes[, xnodes, nodes]) of the oracle, computed once per window"""
    key = (c.pi, c.a, c.L, trellis)
    if key not in _oracle:
        p, seq = bec.window(c)
        score, xn, nd = orc.path(p.prof, bec.xt_of(orc, c.L), seq)
        _oracle[key] = (score,) + orc.unzip(p.K, c.L, xn, nd) + ((xn, nd) if trellis else ())
    return _oracle[key]


def same_steps(r, want):
    return bits(r["score"]) == bits(want[0]) and np.array_equal(r["state_ids"], want[1]) and \
        np.array_equal(r["seqsizes"], want[2])


@pytest.fixture(scope="module")
def reserved(orc):
    eng = load_engine(orc, reserve=1 << 30)
    yield eng
    eng.close()


@pytest.mark.parametrize("B", bec.BLOCKS)
def test_every_window_in_every_launch_form(orc, reserved, monkeypatch, B):
    eng = reserved
    cases = bec.cases(B, gpu=True)
    wins = windows_of(cases)
    want = [oracle_of(orc, c) for c in cases]
    strip = [c for c in cases if bec.profiles()[c.pi].cls == bec.STRIP]
    in_blocks = [c for c in strip if table_bytes(c.L, bec.profiles()[c.pi].K) > MB]
    assert len(strip) == 2 * len(bec.block_lengths(B)) and len(in_blocks) >= len(strip) // 2
    assert {c.L % 5 for c in in_blocks if num_blocks(c.L, B) >= 2} == set(range(5))
    for what, env in FORMS:
        set_form(monkeypatch, B, env)
        t0 = time.perf_counter()
        res = eng.path(wins, trellis=False)
        print(f"B={B}, {what}: {len(wins)} windows in {1e3 * (time.perf_counter() - t0):.0f} ms, redone {eng.path_redone}, "
              f"blocked {eng.path_blocked}")
        for c, r, w in zip(cases, res, want):
            assert same_steps(r, w), (what, bec.profiles()[c.pi].cls, bec.profiles()[c.pi].K, c)
        assert eng.path_redone == 0, what
        assert eng.path_blocked == (len(in_blocks) if env else 0), what


@pytest.mark.parametrize("B", bec.BLOCKS)
def test_the_literal_pass_at_every_residue(orc, monkeypatch, B):
    """trellis=True: one window per class at each residue of L mod 5, in blocks in the fast pass, and the strip class
    (block_edge_cases.literal_rows: 56 .. 75 rows) under a budget that holds a block's table, checkpoints and scratch
    and not a whole table -- its trellis is replayed block by block.  Every xnodes and nodes word, and the steps of
    both passes."""
    cases = bec.literal_subset(B)
    strip = [c for c in cases if bec.profiles()[c.pi].cls == bec.STRIP]
    assert len(strip) == (5 if B == 5 else 10) and {c.L % 5 for c in strip} == set(range(5))
    assert all(num_blocks(c.L, B) >= 2 for c in cases)
    assert len(cases) - len(strip) == 5 * len({c.pi for c in cases if c not in strip}) == 5 * 11
    budget = bec.literal_rows(B)[1]
    assert all(literal_bytes(c.L, bec.profiles()[c.pi].K, B, 1) <= budget * MB < table_bytes(c.L, bec.profiles()[c.pi].K)
               for c in strip)
    set_form(monkeypatch, B, {"DECIPHON_HIP_PATH_BUDGET_MB": str(budget)})
    eng = load_engine(orc)  # a fresh arena: the budget bounds what it places
    try:
        t0 = time.perf_counter()
        res = eng.path(windows_of(cases), trellis=True)
        print(f"B={B}: literal pass of {len(cases)} windows in {1e3 * (time.perf_counter() - t0):.0f} ms, budget {budget} MB, "
              f"placed {eng.path_table_bytes / MB:.1f} MB, blocked {eng.path_blocked}")
        assert eng.path_blocked == len(strip)
        assert 0 < eng.path_table_bytes <= budget * MB
        for c, r in zip(cases, res):
            score, ids, sizes, xn, nd = oracle_of(orc, c, trellis=True)
            what = (bec.profiles()[c.pi].cls, bec.profiles()[c.pi].K, c)
            assert same_steps(r, (score, ids, sizes)), what
            assert np.array_equal(r["xnodes"], xn) and np.array_equal(r["nodes"], nd), what
            assert bits(r["literal_score"]) == bits(score), what
            assert np.array_equal(r["literal_state_ids"], ids) and np.array_equal(r["literal_seqsizes"], sizes), what
    finally:
        eng.close()
