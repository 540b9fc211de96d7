"""GPU: the cases of tests/test_emul_row_loop_ends.py through Engine.cost and Engine.path, bit for bit: short windows
(every length up to twelve rows, every residue of L mod 5 around larger lengths) through every single-wave shape
and every pack shape, packs whose windows end at different rows, and finite junk at k = 0 of MM, MD, IM, DM, DD,
which must leave scores and paths what they are with +inf there.

Which kernels that is: every request here that runs one window per wavefront mixes the single-wave classes and is
small, so its windows of up to 256 positions (Q = 1..4) all run in the fused kernel, dcp_cost_kernel_fused -- never in
dcp_cost_kernel<1..4,1> -- and those above in the narrow kernels <5,1>, <7,1>, <10,1> and the class kernels <6,1>,
<8,1>.  The same windows through each class kernel by itself, with the engine saying which kernel ran:
tests/test_gpu_cost_routes.py."""
import numpy as np
import pytest

from dcp_testlib import bits, random_seq, synth_profile
from delete_run_cases import SINGLE_WAVE
from row_loop_cases import K0_JUNK, WINDOW_LENGTHS, with_k0
from test_gpu_delete_runs import PACK_KS

pytestmark = pytest.mark.gpu


def load(engine, profs, reads):
    engine.clear_profiles()
    for p in profs:
        engine.add_profile(p.K, p.trans, p.match, p.null, p.bg)
    engine.commit()
    engine.set_sequences(reads)
    engine.set_mode(True, False)


def check(orc, profs, reads, wins, nul, alt, what):
    for i, (pi, si, a, b) in enumerate(wins):
        seq = np.ascontiguousarray(reads[si][a:b])
        xt = orc.xtrans(max(len(seq) // 3, 1), True, False)
        assert bits(nul[i]) == bits(orc.null(profs[pi], xt, seq)), (what, profs[pi].K, wins[i])
        assert bits(alt[i]) == bits(orc.cost(profs[pi], xt, seq)), (what, profs[pi].K, wins[i])


def check_paths(orc, profs, reads, wins, res, what):
    for w, r in zip(wins, res):
        pi, si, a, b = w
        seq = np.ascontiguousarray(reads[si][a:b])
        score, xo, no = orc.path(profs[pi], orc.xtrans(max(len(seq) // 3, 1), True, False), seq)
        assert bits(r["score"]) == bits(score), (what, profs[pi].K, w)
        assert np.array_equal(r["xnodes"], xo) and np.array_equal(r["nodes"], no), (what, profs[pi].K, w)
        # the steps of the fast pass (the table-writing kernels share the cost kernels' row loop) against the oracle's
        ids, sizes = orc.unzip(profs[pi].K, len(seq), xo, no)
        assert np.array_equal(r["state_ids"], ids) and np.array_equal(r["seqsizes"], sizes), (what, profs[pi].K, w)


def test_short_windows_single_wave_shapes(engine, orc, monkeypatch):
    """all 18 profiles in one request: a small mix of classes, so Q = 1..4 run in the fused kernel (see above)"""
    monkeypatch.setenv("DECIPHON_HIP_PACK", "0")  # K <= 124 too on a wavefront of its own
    rng = np.random.default_rng(801)
    profs = [synth_profile(rng, K, [None, 2.0][Q % 2]) for Q, K in SINGLE_WAVE]
    reads = [random_seq(rng, max(WINDOW_LENGTHS)) for _ in profs]
    load(engine, profs, reads)
    # windows from the read's start and windows that end at its end: different code rows for the same length
    wins = [(i, i, 0, L) for i in range(len(profs)) for L in WINDOW_LENGTHS]
    wins += [(i, i, len(reads[i]) - L, len(reads[i])) for i in range(len(profs)) for L in WINDOW_LENGTHS[:17]]
    nul, alt = engine.cost(wins)
    check(orc, profs, reads, wins, nul, alt, "single wave")
    # the table-writing kernels share the row loop: a few short windows per class through the path pass
    some = [w for w in wins if w[3] - w[2] in (1, 4, 5, 6, 11, 35) and w[2] == 0]
    check_paths(orc, profs, reads, some, engine.path(some), "single wave")


def pack_case(rng, lengths):
    profs = [synth_profile(rng, K, [None, 1.0][K % 2]) for K in PACK_KS]
    reads = [random_seq(rng, max(lengths)) for _ in profs]
    return profs, reads


def cost_three_ways(engine, monkeypatch, wins):
    """packed with the LDS tables, packed from global memory, one window per wavefront"""
    monkeypatch.delenv("DECIPHON_HIP_PACK", raising=False)
    monkeypatch.delenv("DECIPHON_HIP_PACK_LDS", raising=False)
    packed = engine.cost(wins)
    monkeypatch.setenv("DECIPHON_HIP_PACK_LDS", "0")
    nolds = engine.cost(wins)
    monkeypatch.delenv("DECIPHON_HIP_PACK_LDS")
    monkeypatch.setenv("DECIPHON_HIP_PACK", "0")
    plain = engine.cost(wins)
    monkeypatch.delenv("DECIPHON_HIP_PACK")
    return (("packed", packed), ("packed, tables in global memory", nolds), ("plain", plain))


def test_short_windows_pack_shapes(engine, orc, monkeypatch):
    """every window of a call has the same length: a pack's row loop ends where all its groups end"""
    rng = np.random.default_rng(802)
    profs, reads = pack_case(rng, WINDOW_LENGTHS[:22])
    load(engine, profs, reads)
    for L in WINDOW_LENGTHS[:22]:
        # seventeen windows per profile: full packs and a partly filled one for every group count
        wins = [(i, i, a, a + L) for i in range(len(profs)) for a in range(17) if a + L <= len(reads[i])]
        wins = wins or [(i, i, 0, L) for i in range(len(profs))]
        ways = cost_three_ways(engine, monkeypatch, wins)
        for what, (nul, alt) in ways:
            check(orc, profs, reads, wins, nul, alt, (what, L))


def test_windows_that_end_early_in_a_pack(engine, orc, monkeypatch):
    """windows of one profile with lengths 1 .. 40 in one call: the groups of a pack end at different rows and
    capture their results at their own last row"""
    rng = np.random.default_rng(803)
    profs, reads = pack_case(rng, (64,))
    load(engine, profs, reads)
    wins = []
    for i in range(len(profs)):
        for j in range(45):
            a = int(rng.integers(0, 24))
            wins.append((i, i, a, a + int(rng.integers(1, 41))))
    ways = cost_three_ways(engine, monkeypatch, wins)
    for what, (nul, alt) in ways:
        check(orc, profs, reads, wins, nul, alt, what)


def test_junk_at_position_zero(engine, orc, monkeypatch):
    """a profile handed to add_profile with finite junk at k = 0 of MM, MD, IM, DM, DD scores and walks exactly as
    the same profile with +inf there, which in turn equals the oracle -- one window per wavefront and packed"""
    rng = np.random.default_rng(804)
    Ks = sorted({K for _, K in SINGLE_WAVE} | set(PACK_KS))
    bases = [synth_profile(rng, K, [None, 1.0][K % 2]) for K in Ks]
    forms = (None,) + K0_JUNK
    profs = [with_k0(b, j) for b in bases for j in forms]  # profile index = base * len(forms) + form
    reads = [random_seq(rng, int(rng.integers(30, 60))) for _ in bases]
    load(engine, profs, reads)
    F = len(forms)
    cuts = (1, 7, 25)
    wins = [(bi * F + f, bi, 0, min(c, len(reads[bi]))) for bi in range(len(bases)) for f in range(F) for c in cuts]
    wins += [(bi * F + f, bi, 0, len(reads[bi])) for bi in range(len(bases)) for f in range(F)]
    for what, (nul, alt) in cost_three_ways(engine, monkeypatch, wins):
        clean = [i for i, w in enumerate(wins) if w[0] % F == 0]
        check(orc, profs, reads, [wins[i] for i in clean], nul[clean], alt[clean], what)
        # every junk form against the +inf form of the same profile and window
        by = {}
        for i, w in enumerate(wins):
            by.setdefault((w[0] // F, w[1], w[2], w[3]), []).append(i)
        for key, idx in by.items():
            assert len(idx) == F
            for i in idx[1:]:
                assert bits(nul[i]) == bits(nul[idx[0]]) and bits(alt[i]) == bits(alt[idx[0]]), (what, key, wins[i])
    full = [w for w in wins if w[3] == len(reads[w[1]])]
    res = engine.path(full)
    check_paths(orc, profs, reads, [w for w in full if w[0] % F == 0], [r for w, r in zip(full, res) if w[0] % F == 0],
                "+inf at k = 0")
    first = {}
    for w, r in zip(full, res):
        ref = first.setdefault(w[0] // F, r)
        assert bits(r["score"]) == bits(ref["score"]), w
        assert r["xnodes"].tobytes() == ref["xnodes"].tobytes() and r["nodes"].tobytes() == ref["nodes"].tobytes(), w
        assert r["state_ids"].tobytes() == ref["state_ids"].tobytes(), w
        assert r["seqsizes"].tobytes() == ref["seqsizes"].tobytes(), w
