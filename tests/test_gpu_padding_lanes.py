"""GPU: lanes beyond a profile's K positions read an emission row with the last lane that owns a position
(deciphon_amd/csrc/dcp_types.h, "which columns of an emission row a lane reads") instead of their +inf padding
columns.  Engine.cost against the oracle bit for bit on windows of 3, 7 and 60 rows, on tables with the structure of
real models (the minifam seeds tiled to K nodes), at the core sizes where the rule has the most and the least to do:

  one window per wavefront, Q = 2..8 and 10 positions per lane: K = 64 (Q - 1) + 1 (the fewest lanes with a position),
  K = 64 Q - 1 (the last lane straddles K), K = 64 Q (no padding) and one K between them that Q does not divide; the
  K <= 320, <= 448 and <= 640 among them take the narrow kernels (5,1), (7,1), (10,1) on a wider profile's table, with
  the cost-order copy and without it, and the class's own kernel (6,1), (8,1) with DECIPHON_HIP_NARROW=0;

  packs, every shape: the smallest K routed to it, K = (S - 1) Q, one K that Q does not divide, window lengths that
  differ within a pack -- from LDS tables, from global memory and against one window per wavefront;

  the fast path pass (its checkpoint pass shares the cost kernels' set-up and reads the same way; the table-writing
  kernels beside it keep every lane's own columns): one window with a planted domain per Q in {2, 3, 5, 8} at the K
  with the fewest lanes, two blocks long, its steps against the oracle's."""
import os

import numpy as np
import pytest

from dcp_testlib import GOLDEN, bits

pytestmark = pytest.mark.gpu

ROWS = (3, 7, 60)

# Q -> the four core sizes (fewest lanes, one Q does not divide, the last lane straddles K, no padding)
SINGLE = {2: (65, 99, 127, 128), 3: (129, 160, 191, 192), 4: (193, 230, 255, 256), 5: (257, 291, 319, 320),
          6: (321, 350, 383, 384), 7: (385, 415, 447, 448), 8: (449, 485, 511, 512), 10: (577, 605, 639, 640)}

# (Q, S) of every pack shape in the order a core size is routed (the first that holds it), with its capacity
PACK_SHAPES = ((1, 4), (2, 4), (4, 4), (2, 8), (4, 8), (2, 16), (3, 16), (4, 16), (2, 32), (3, 32), (4, 32))


def pack_core_sizes():
    """per shape: the smallest K routed to it, K = (S - 1) Q, and the largest K between them that Q does not divide
    (with two positions per lane and room for two sizes only, that is the smallest itself)"""
    out, prev = [], 0
    for Q, S in PACK_SHAPES:
        cap = (S - 1) * Q
        odd = [K for K in range(prev + 1, cap) if K % Q]
        out.append(((Q, S), tuple(sorted({prev + 1, cap} | set(odd[-1:])))))
        prev = cap
    return out


@pytest.fixture(scope="module")
def seeds():
    from deciphon_amd import synth

    return synth.load_seeds(os.path.join(GOLDEN, "minifam.dcp"))


def tiled(seeds, orc, K, offset):
    """a protein of K nodes with the structure of real models, and the oracle's profile of it"""
    from deciphon_amd import synth
    from oracle.dcp_reader import Protein

    p = synth.tile_protein(seeds, K, offset, f"T{K}")
    prof = orc.setup_profile(Protein(p["accession"], 1, p["consensus"], p["core_size"], p["null_emission"],
                                     p["bg_emission"], p["trans"], p["emission"], p["BMk"]))
    return p, prof


def domain_read(p, rng, n):
    """n nucleotides: a mutated stretch of the protein's own consensus, random beyond it"""
    from deciphon_amd import synth

    dom = synth.mutate(synth.back_translate(p["consensus"][: n // 3]), rng, 0.06, 0.02, 0.02)[:n]
    x = rng.integers(0, 4, size=n).astype(np.uint8)
    x[: len(dom)] = dom
    return x


def load(engine, prots, reads):
    engine.clear_profiles()
    for p in prots:
        engine.add_protein(p["core_size"], p["trans"], p["emission"], p["BMk"], p["null_emission"], p["bg_emission"])
    engine.commit()
    engine.set_sequences(reads)
    engine.set_mode(True, False)


def reference(orc, profs, reads, wins):
    """(null, cost) of every window by the oracle, computed once per test"""
    out = []
    for pi, si, a, b in wins:
        seq = np.ascontiguousarray(reads[si][a:b])
        xt = orc.xtrans(max(len(seq) // 3, 1), True, False)
        out.append((bits(orc.null(profs[pi], xt, seq)), bits(orc.cost(profs[pi], xt, seq))))
    return out


def check(want, wins, profs, got, what):
    nul, alt = got
    for i, w in enumerate(wins):
        assert (bits(nul[i]), bits(alt[i])) == want[i], (what, profs[w[0]].K, w)


@pytest.mark.parametrize("Q", sorted(SINGLE))
def test_single_wave(engine, orc, seeds, monkeypatch, Q):
    rng = np.random.default_rng(1200 + Q)
    made = [tiled(seeds, orc, K, 7 * i + Q) for i, K in enumerate(SINGLE[Q])]
    prots, profs = [m[0] for m in made], [m[1] for m in made]
    reads = [domain_read(p, rng, 72) for p in prots]
    wins = [(i, i, a, a + L) for i in range(len(prots)) for L in ROWS for a in (0, 9)]
    want = reference(orc, profs, reads, wins)
    monkeypatch.setenv("DECIPHON_HIP_PACK", "0")  # (nothing here is short enough for a pack; keeps it so)
    load(engine, prots, reads)
    check(want, wins, profs, engine.cost(wins), "default kernels")
    if Q in (5, 7, 10):
        # the class's own kernel -- (6,1), (8,1), (6,2) -- on the same profiles: still fewer lanes with a position
        monkeypatch.setenv("DECIPHON_HIP_NARROW", "0")
        check(want, wins, profs, engine.cost(wins), "narrow kernels off")
        monkeypatch.delenv("DECIPHON_HIP_NARROW")
    if Q in (5, 10):
        # the narrow kernel on the canonical rows instead of the cost-order copy (decided when profiles are staged)
        monkeypatch.setenv("DECIPHON_HIP_COST_ORDER", "0")
        load(engine, prots, reads)
        check(want, wins, profs, engine.cost(wins), "no cost-order copy")


@pytest.mark.parametrize("shape,Ks", pack_core_sizes(), ids=[f"{Q}x{S}" for Q, S in PACK_SHAPES])
def test_packs(engine, orc, seeds, monkeypatch, shape, Ks):
    Q, S = shape
    assert len(Ks) >= 2 and all(K <= (S - 1) * Q for K in Ks)
    assert Q == 1 or any(K % Q for K in Ks)
    rng = np.random.default_rng(1300 + 40 * Q + S)
    made = [tiled(seeds, orc, K, 5 * i + S) for i, K in enumerate(Ks)]
    prots, profs = [m[0] for m in made], [m[1] for m in made]
    reads = [domain_read(p, rng, 80) for p in prots]
    # nineteen windows per profile, lengths 3, 7 and 60 in turn: no group count divides it, and the windows that
    # share a wavefront differ in length
    wins = [(i, i, j, j + ROWS[j % 3]) for i in range(len(prots)) for j in range(19)]
    want = reference(orc, profs, reads, wins)
    load(engine, prots, reads)
    monkeypatch.delenv("DECIPHON_HIP_PACK", raising=False)
    monkeypatch.delenv("DECIPHON_HIP_PACK_LDS", raising=False)
    check(want, wins, profs, engine.cost(wins), "packed")
    monkeypatch.setenv("DECIPHON_HIP_PACK_LDS", "0")
    check(want, wins, profs, engine.cost(wins), "packed, tables in global memory")
    monkeypatch.delenv("DECIPHON_HIP_PACK_LDS")
    monkeypatch.setenv("DECIPHON_HIP_PACK", "0")
    check(want, wins, profs, engine.cost(wins), "one window per wavefront")


def test_fast_path_pass(engine, orc, seeds, monkeypatch):
    for v in ("DECIPHON_HIP_PACK", "DECIPHON_HIP_NARROW", "DECIPHON_HIP_COST_ORDER", "DECIPHON_HIP_PATH"):
        monkeypatch.delenv(v, raising=False)
    rng = np.random.default_rng(1400)
    Ks = [SINGLE[Q][0] for Q in (2, 3, 5, 8)]
    made = [tiled(seeds, orc, K, 3 * i) for i, K in enumerate(Ks)]
    prots, profs = [m[0] for m in made], [m[1] for m in made]
    reads = []
    for p in prots:  # 600 rows: two blocks of the default 500, so the checkpoint kernels run too
        x = rng.integers(0, 4, size=600).astype(np.uint8)
        dom = domain_read(p, rng, 360)
        x[120 : 120 + len(dom)] = dom
        reads.append(x)
    load(engine, prots, reads)
    wins = [(i, i, 0, 600) for i in range(len(prots))]
    res = engine.path(wins, trellis=False)
    assert engine.path_redone == 0  # the fast pass itself, not the literal kernel behind it
    for (pi, si, a, b), r in zip(wins, res):
        seq = np.ascontiguousarray(reads[si][a:b])
        score, xo, no = orc.path(profs[pi], orc.xtrans(max(len(seq) // 3, 1), True, False), seq)
        ids, sizes = orc.unzip(profs[pi].K, len(seq), xo, no)
        assert bits(r["score"]) == bits(score), profs[pi].K
        assert np.array_equal(r["state_ids"], ids) and np.array_equal(r["seqsizes"], sizes), profs[pi].K
