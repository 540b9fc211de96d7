"""GPU: the cases of tests/test_emul_delete_runs.py -- profiles whose best alignment deletes a planted run of
1 .. K - 2 positions (tests/delete_run_cases.py) -- through Engine.cost, bit for bit against the oracle: every
single-wave kernel (1..8 and 10 positions per lane) at both ends of the profiles it serves, and every pack shape
with windows of different lengths in one pack, packed with and without the LDS tables and one window per wavefront.
One path call per class: the table-writing kernels of the path pass share the cost kernels' row().

Which kernels that is: test_single_wave_shapes sends one core size per request, so it runs the class kernels
dcp_cost_kernel<1..4,1>, <6,1>, <8,1> and the narrow kernels <5,1>, <7,1>, <10,1>, never the fused kernel and never the
class kernel of 513..640 positions, <6,2>; the "plain" requests of test_pack_shapes_with_mixed_window_lengths mix classes
0 and 1 and are small, so they run in the fused kernel, not in <1,1> and <2,1>.  Every kernel by itself on these runs,
with the engine saying which one ran: tests/test_gpu_cost_routes.py."""
import numpy as np
import pytest

from dcp_testlib import bits
from delete_run_cases import DD_KINDS, LONG_RUN, SINGLE_WAVE, planted, run_lengths, single_wave_cases

pytestmark = pytest.mark.gpu

# K at the upper and the lower end of every pack shape's capacity (3, 6, 12, 14, 28, 45, 60, 93, 124 positions)
PACK_KS = (3, 4, 6, 7, 12, 13, 14, 15, 28, 29, 45, 46, 60, 61, 93, 94, 124)


def load(engine, orc, profs, reads, quant):
    engine.clear_profiles()
    for p in profs:
        engine.add_profile(p.K, p.trans, p.match, p.null, p.bg)
    engine.commit()
    engine.set_sequences(reads)
    engine.set_mode(True, False)
    if quant:
        smax = max(len(r) // 3 for r in reads) + 1
        table = np.zeros((smax + 1, 13), np.float32)
        for s in range(1, smax + 1):
            table[s] = (np.round(orc.xtrans(s, True, False) / quant) * quant).astype(np.float32)
        engine.set_xtrans_table(table)


def xtrans(orc, n, quant):
    xt = orc.xtrans(max(n // 3, 1), True, False)
    return (np.round(xt / quant) * quant).astype(np.float32) if quant else xt


def check(orc, profs, reads, wins, nul, alt, quant, what):
    for i, (pi, si, a, b) in enumerate(wins):
        seq = np.ascontiguousarray(reads[si][a:b])
        xt = xtrans(orc, len(seq), quant)
        assert bits(nul[i]) == bits(orc.null(profs[pi], xt, seq)), (what, profs[pi].K, wins[i])
        assert bits(alt[i]) == bits(orc.cost(profs[pi], xt, seq)), (what, profs[pi].K, wins[i])


@pytest.mark.parametrize("Q,K", SINGLE_WAVE)
def test_single_wave_shapes(engine, orc, monkeypatch, Q, K):
    monkeypatch.setenv("DECIPHON_HIP_PACK", "0")  # K <= 124 too on a wavefront of its own: the (1,1) and (2,1) kernels
    rng = np.random.default_rng(1000 + K)
    cases = [c for c in single_wave_cases() if c[0] == Q and c[1] == K]
    assert len(cases) == 6 * len(run_lengths(K))
    try:
        for quant in sorted({c[4] for c in cases}, key=lambda q: q or 0.0):
            runs = [r for _, _, r, _, q in cases if q == quant]
            made = [planted(rng, K, r, dd, quant) for _, _, r, dd, q in cases if q == quant]
            profs, reads = [m[0] for m in made], [m[1] for m in made]
            load(engine, orc, profs, reads, quant)
            wins = [(i, i, 0, len(reads[i])) for i in range(len(made))]
            nul, alt = engine.cost(wins)
            check(orc, profs, reads, wins, nul, alt, quant, (Q, K))
            if not quant:  # one path call per class: a free run over up to half of the profile
                i = runs.index(max(r for r in runs if r <= max(K // 2, 1)))
                res = engine.path([wins[i]])
                score, xo, no = orc.path(profs[i], xtrans(orc, len(reads[i]), None), reads[i])
                assert bits(res[0]["score"]) == bits(score), (Q, K, i)
                assert np.array_equal(res[0]["xnodes"], xo) and np.array_equal(res[0]["nodes"], no), (Q, K, i)
    finally:
        engine.set_xtrans_table(np.zeros((0, 13), np.float32))


@pytest.mark.parametrize("quant", [None, 2.0])
def test_pack_shapes_with_mixed_window_lengths(engine, orc, monkeypatch, quant):
    rng = np.random.default_rng(77 if quant else 76)
    profs, reads, wins = [], [], []
    for K in PACK_KS:
        for r in run_lengths(K):
            for dd in DD_KINDS:
                prof, seq, a = planted(rng, K, r, dd, quant)
                pi = len(profs)
                profs.append(prof)
                reads.append(seq)
                # the full read, the read cut short in front of, inside and behind the run, and -- thirteen windows per
                # profile, which no pack's group count divides -- the full read again
                for cut in (len(seq), 3 * a, len(seq) - 3, 3 * a + 6, len(seq) // 2 + 1) + (len(seq),) * 8:
                    wins.append((pi, pi, 0, max(1, min(cut, len(seq)))))
    assert 3 * sum(r >= LONG_RUN for K in PACK_KS for r in run_lengths(K)) >= sum(len(run_lengths(K)) for K in PACK_KS)
    load(engine, orc, profs, reads, quant)
    try:
        monkeypatch.delenv("DECIPHON_HIP_PACK", raising=False)
        monkeypatch.delenv("DECIPHON_HIP_PACK_LDS", raising=False)
        packed = engine.cost(wins)
        monkeypatch.setenv("DECIPHON_HIP_PACK_LDS", "0")
        nolds = engine.cost(wins)
        monkeypatch.delenv("DECIPHON_HIP_PACK_LDS")
        monkeypatch.setenv("DECIPHON_HIP_PACK", "0")
        plain = engine.cost(wins)
        monkeypatch.delenv("DECIPHON_HIP_PACK")
        for what, (nul, alt) in (("packed", packed), ("packed, tables in global memory", nolds), ("plain", plain)):
            check(orc, profs, reads, wins[::13] if what != "packed" else wins, nul[::13] if what != "packed" else nul,
                  alt[::13] if what != "packed" else alt, quant, what)
            assert np.array_equal(nul.view(np.uint32), packed[0].view(np.uint32)), what
            assert np.array_equal(alt.view(np.uint32), packed[1].view(np.uint32)), what
    finally:
        engine.set_xtrans_table(np.zeros((0, 13), np.float32))
