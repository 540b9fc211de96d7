"""GPU: the limits of the step buffers of the path pass.  A path of N steps fits a buffer of N and not of N - 1: the
rule is `n + 1 >= cap` in the traceback of the fast pass (deciphon_amd/csrc/traceback.h), where n survives the hand-over
from block to block in DcpTraceState::n, and again in the device unzip of the literal pass; a path that fits neither is
unzipped on the host.  Steps are written from the end of a window's buffer backwards and the buffers lie side by side,
so a walk that went one word too far would overwrite the last step of the window in front of it.

One request of windows of four blocks (DECIPHON_HIP_CKPT_ROWS=10, 38 rows) of a single-wave class, a multi-wave class
and the strip class, all path lengths distinct, under DECIPHON_HIP_UNZIP_CAP = c for c at and one below the shortest
path, the longest and the median of each class: whichever route a window took, its steps are the oracle's, and the fast pass gave up
exactly the windows with N > c.  The engine takes the slowest windows first, in a stable sort by rows and class
(engine_path.cpp, path_run): the windows of a class have the same length here, so they keep the order of the request,
in which long and short paths alternate -- every overflowing window but the first of its class has a fitting one in front
of it at some c."""
import time

import numpy as np
import pytest

import block_edge_cases as bec
from path_layout import MB, num_blocks, table_bytes
from test_gpu_block_edges import load_engine, oracle_of, same_steps, set_form, windows_of

pytestmark = pytest.mark.gpu

B = 10
ROWS = 3 * B + 8       # four blocks
PER_CLASS = 7
CLASS_KS = (257, 1025, 6144)  # (6,1), (6,4) and the strip class: the profiles with cheap delete runs, paths of many sizes
SMALL = {"DECIPHON_HIP_PATH_BUDGET_MB": "1"}  # the strip windows in blocks (tests/test_gpu_block_edges.py)
FORMS = (("one launch per window", SMALL),
         ("three blocks side by side", dict(SMALL, DECIPHON_HIP_PATH_GROUP="3")),
         ("a launch per block and phase", dict(SMALL, DECIPHON_HIP_PATH_GROUP="1", DECIPHON_HIP_PATH_FUSED="0")))


def limit_cases(orc):
    """-> ([Case], [N]): per class PER_CLASS windows of ROWS rows at different places of the read, every N distinct, in the
    order longest, shortest, second longest, second shortest .."""
    taken, cases, steps = set(), [], []
    for K in CLASS_KS:
        (pi,) = [i for i, p in enumerate(bec.profiles()) if p.K == K and not p.emul]
        assert bec.profiles()[pi].kind == "deletes"
        by_n = {}
        for a in range(bec.READ - ROWS + 1):
            c = bec.Case(pi, B, ROWS, a, bec.mode_of(ROWS))
            n = len(oracle_of(orc, c)[1])
            if n not in taken:
                by_n.setdefault(n, c)
        ns = sorted(by_n)
        assert len(ns) >= PER_CLASS, (K, ns)
        pick = [ns[round(i * (len(ns) - 1) / (PER_CLASS - 1))] for i in range(PER_CLASS)]
        assert len(set(pick)) == PER_CLASS
        taken |= set(pick)
        order = [pick[-1 - i // 2] if i % 2 == 0 else pick[i // 2] for i in range(PER_CLASS)]
        cases += [by_n[n] for n in order]
        steps += order
    return cases, steps


def capacities(steps):
    """at and one below the shortest path, the longest, and the median of every class (the last window of a class in
    the request: the one in front of it is the next shorter of the class)"""
    mid = [sorted(steps[k * PER_CLASS : (k + 1) * PER_CLASS])[PER_CLASS // 2] for k in range(len(CLASS_KS))]
    return sorted({c for n in [min(steps), max(steps)] + mid for c in (n - 1, n)})


@pytest.fixture(scope="module")
def loaded(orc):
    eng = load_engine(orc, reserve=256 * MB)
    cases, steps = limit_cases(orc)
    yield eng, cases, steps
    eng.close()


def test_the_request_is_what_the_limits_need(loaded):
    _, cases, steps = loaded
    assert len(cases) == len(CLASS_KS) * PER_CLASS == len(set(steps)) and num_blocks(ROWS, B) == 4
    for k in range(len(CLASS_KS)):
        part = steps[k * PER_CLASS : (k + 1) * PER_CLASS]
        assert all((a > b) == (i % 2 == 0) for i, (a, b) in enumerate(zip(part, part[1:]))), part
    assert all(table_bytes(ROWS, K) > MB for K in CLASS_KS if K > 4096)
    caps = capacities(steps)
    assert 6 <= len(caps) <= 10 and min(caps) == min(steps) - 1 and max(caps) == max(steps)
    # some capacity leaves a window overflowing right behind one that fits, in every class
    for k in range(len(CLASS_KS)):
        part = steps[k * PER_CLASS : (k + 1) * PER_CLASS]
        assert any(a <= c < b for c in caps for a, b in zip(part, part[1:])), (part, caps)


@pytest.mark.parametrize("form", range(len(FORMS)), ids=[f[0] for f in FORMS])
def test_a_path_fits_its_length_and_not_one_less(orc, loaded, monkeypatch, form):
    eng, cases, steps = loaded
    what, env = FORMS[form]
    wins = windows_of(cases)
    want = [oracle_of(orc, c) for c in cases]
    nstrip = sum(1 for c in cases if bec.profiles()[c.pi].cls == bec.STRIP)

    def run(cap):
        set_form(monkeypatch, B, dict(env, DECIPHON_HIP_UNZIP_CAP=str(cap)) if cap else env)
        t0 = time.perf_counter()
        res = eng.path(wins, trellis=False)
        ms = 1e3 * (time.perf_counter() - t0)
        for i, (c, r, w) in enumerate(zip(cases, res, want)):
            assert same_steps(r, w), (what, cap, i, steps[i], c)
            packed = eng.path_steps_packed(i)
            assert np.array_equal(packed, w[1].astype(np.uint32) | (w[2].astype(np.uint32) << 16)), (what, cap, i)
        assert eng.path_blocked == nstrip, (what, cap)
        return eng.path_redone, ms

    redone, ms = run(0)
    print(f"{what}: default capacity {ms:.0f} ms, redone {redone}")
    assert redone == 0
    for cap in capacities(steps):
        redone, ms = run(cap)
        print(f"{what}: capacity {cap}: {ms:.0f} ms, redone {redone} of {len(cases)}")
        assert redone == sum(1 for n in steps if n > cap), (what, cap, sorted(steps))
