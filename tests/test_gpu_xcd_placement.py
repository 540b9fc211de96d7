"""GPU: the cost kernels of a class take their windows in the plain order or in eighths of the list, one eighth per
XCD (deciphon_amd/csrc/dcp_types.h, "which XCD's L2 serves which windows"), as dcp_xcd_placement decides per launch or
as DECIPHON_HIP_XCD_PLACEMENT = plain | eighths | auto tells.  Where a workgroup runs decides nothing: Engine.cost must
return the same bits for every window under all three, and the oracle's.

Two profiles each at K = 322, 400, 500 and 600 -- the kernels (6,1), (7,1), (8,1) and (10,1): each narrow kernel and
two that are their class's own -- and launches of 1, 7, 9, 16 and 23 windows per kernel: fewer windows than XCDs, every
kind of remainder of the eighths (none, one, seven; shares of 0, 1, 2 and 3 windows), and, from 7 windows on, the
boundary between the two profiles inside the list.  Windows are 24 to 45 nucleotides of reads of 64, given to the
engine in an order that is not the list's, so a window dropped, scored twice or written to another window's slot
shows."""
import os

import numpy as np
import pytest

from dcp_testlib import GOLDEN, bits

pytestmark = pytest.mark.gpu

CORE_SIZES = (322, 322, 400, 400, 500, 500, 600, 600)
LAUNCH_WINDOWS = (1, 7, 9, 16, 23)
LENGTHS = (24, 45, 31, 36)
KNOB = "DECIPHON_HIP_XCD_PLACEMENT"


def windows_of(n):
    """n windows for each pair of profiles of one core size (one launch each), the second profile's interleaved with
    the first's"""
    wins = []
    for pair in range(len(CORE_SIZES) // 2):
        for j in range(n):
            p = 2 * pair + (j % 2 if n > 1 else 0)
            L = LENGTHS[(j + pair) % len(LENGTHS)]
            a = (5 * j + pair) % (64 - L + 1)
            wins.append((p, p, a, a + L))
    return wins


@pytest.fixture(scope="module")
def setup(engine, orc):
    from deciphon_amd import synth
    from oracle.dcp_reader import Protein

    seeds = synth.load_seeds(os.path.join(GOLDEN, "minifam.dcp"))
    rng = np.random.default_rng(1400)
    prots, profs, reads = [], [], []
    for i, K in enumerate(CORE_SIZES):
        p = synth.tile_protein(seeds, K, 11 * i + 3, f"X{K}_{i}")
        prots.append(p)
        profs.append(orc.setup_profile(Protein(p["accession"], 1, p["consensus"], p["core_size"], p["null_emission"],
                                               p["bg_emission"], p["trans"], p["emission"], p["BMk"])))
        dom = synth.mutate(synth.back_translate(p["consensus"][:21]), rng, 0.06, 0.02, 0.02)[:64]
        x = rng.integers(0, 4, size=64).astype(np.uint8)
        x[: len(dom)] = dom
        reads.append(x)
    want = {}  # the oracle's (null, cost) bits of every distinct window, computed once
    for n in LAUNCH_WINDOWS:
        for w in windows_of(n):
            if w not in want:
                seq = np.ascontiguousarray(reads[w[1]][w[2]:w[3]])
                xt = orc.xtrans(max(len(seq) // 3, 1), True, False)
                want[w] = (bits(orc.null(profs[w[0]], xt, seq)), bits(orc.cost(profs[w[0]], xt, seq)))
    return prots, reads, want


@pytest.fixture()
def loaded(engine, setup, monkeypatch):
    for v in ("DECIPHON_HIP_PACK", "DECIPHON_HIP_NARROW", "DECIPHON_HIP_COST_ORDER", KNOB):
        monkeypatch.delenv(v, raising=False)
    prots, reads, want = setup
    engine.clear_profiles()
    for p in prots:
        engine.add_protein(p["core_size"], p["trans"], p["emission"], p["BMk"], p["null_emission"], p["bg_emission"])
    engine.commit()
    engine.set_sequences(reads)
    engine.set_mode(True, False)
    return engine, want


@pytest.mark.parametrize("n", LAUNCH_WINDOWS)
def test_same_bits_wherever_a_window_runs(loaded, monkeypatch, n):
    engine, want = loaded
    wins = windows_of(n)
    assert len(wins) == 4 * n
    got = {}
    for mode in ("plain", "eighths", "auto", None):
        if mode is None:
            monkeypatch.delenv(KNOB)
        else:
            monkeypatch.setenv(KNOB, mode)
        nul, alt = engine.cost(wins)
        got[mode] = [(bits(a), bits(b)) for a, b in zip(nul, alt)]
    for mode, res in got.items():
        for w, r, p in zip(wins, res, got["plain"]):
            assert r == p, (mode, "against plain", CORE_SIZES[w[0]], w)
            assert r == want[w], (mode, "against the oracle", CORE_SIZES[w[0]], w)


def test_narrow_kernels_off(loaded, monkeypatch):
    """the class's own kernels -- (6,1), (8,1), (6,2) -- take every window of their class in one launch"""
    engine, want = loaded
    monkeypatch.setenv("DECIPHON_HIP_NARROW", "0")
    wins = windows_of(23)
    for mode in ("plain", "eighths", "auto"):
        monkeypatch.setenv(KNOB, mode)
        nul, alt = engine.cost(wins)
        for w, a, b in zip(wins, nul, alt):
            assert (bits(a), bits(b)) == want[w], (mode, CORE_SIZES[w[0]], w)


def test_knob_refuses_anything_else(loaded, monkeypatch):
    from deciphon_amd.hip import HipError

    engine, want = loaded
    monkeypatch.setenv(KNOB, "quarters")
    with pytest.raises(HipError):
        engine.cost(windows_of(7))
    monkeypatch.setenv(KNOB, "auto")
    wins = windows_of(7)
    nul, alt = engine.cost(wins)  # and the engine goes on
    assert [(bits(a), bits(b)) for a, b in zip(nul, alt)] == [want[w] for w in wins]
