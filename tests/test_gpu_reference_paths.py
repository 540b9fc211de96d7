"""GPU: the steps of engine.path in every path mode the engine picks between, against paths made by the REFERENCE's
own trellis_unzip on the reference's own trellises (tests/golden: synth_ties.npz, large_classes.npz,
minifam_consensus.npz; made by make_golden.py through oracle/_ref), and the engine's special-transition table against
the reference's xtrans.c (reference_walks.npz).  Reads only goldens and, where it was built, oracle/_ref."""
import hashlib
import os
import sys

import numpy as np
import pytest

from dcp_testlib import GOLDEN, bits, random_seq, read_fasta, synth_profile, walks_reflib
from large_cases import build_case, large_cases

sys.path.insert(0, GOLDEN)
from make_golden import MODES, XT_ROWS, synth_case_params, synth_xt  # noqa: E402

pytestmark = pytest.mark.gpu

# the forms of the path pass (deciphon_amd/csrc/engine_path.cpp): blocks side by side (default), checkpoints every 50 rows,
# one workgroup walking its window's blocks (dcp_path_blocks_kernel), a launch per block and phase, and the literal
# pass with the device unzip (dcp_unzip_kernel)
PATH_MODES = {
    "default": {},
    "checkpoints every 50 rows": {"DECIPHON_HIP_CKPT_ROWS": "50"},
    "fused blocks kernel": {"DECIPHON_HIP_PATH_GROUP": "1"},
    "a launch per block": {"DECIPHON_HIP_PATH_GROUP": "1", "DECIPHON_HIP_PATH_FUSED": "0"},
    "literal": {"DECIPHON_HIP_PATH": "literal"},
}


def _golden_path(g, j):
    a, b = int(g["path_off"][j]), int(g["path_off"][j + 1])
    return g["path_ids"][a:b], g["path_sizes"][a:b]


def _same_steps(p, want) -> bool:
    return np.array_equal(p["state_ids"], want[0]) and np.array_equal(p["seqsizes"], want[1])


@pytest.fixture(params=list(PATH_MODES))
def path_mode(request, monkeypatch):
    for k, v in PATH_MODES[request.param].items():
        monkeypatch.setenv(k, v)
    return request.param


def test_tie_rich_paths_are_the_references(engine, orc, path_mode):
    """All 240 tie-rich cases of synth_ties.npz (costs quantised to 0.5 .. 8, K = 2 .. 256): where equal-cost
    predecessors are everywhere, every path mode takes the reference trellis_unzip's path, step for step."""
    g = np.load(os.path.join(GOLDEN, "synth_ties.npz"))
    rng = np.random.default_rng(int(g["seed"]))
    groups = {}
    for it in range(int(g["ncase"])):
        K, L, quant, pinf, mh, h3 = synth_case_params(rng, it)
        prof = synth_profile(rng, K, quant, pinf)
        seq = random_seq(rng, L)
        groups.setdefault((quant, mh, h3), []).append((it, K, L, prof, seq))
    walked = 0
    try:
        for (quant, mh, h3), grp in groups.items():
            engine.clear_profiles()
            for c in grp:
                engine.add_profile(c[3].K, c[3].trans, c[3].match, c[3].null, c[3].bg)
            engine.commit()
            engine.set_sequences([c[4] for c in grp])
            engine.set_mode(bool(mh), bool(h3))
            smax = max(max(c[2] // 3, 1) for c in grp)
            table = np.zeros((smax + 1, 13), np.float32)
            for s in range(1, smax + 1):
                table[s] = synth_xt(orc, 3 * s, mh, h3, quant)
            engine.set_xtrans_table(table)
            hit = [i for i, c in enumerate(grp) if len(_golden_path(g, c[0])[0])]
            paths = engine.path([(i, i, 0, grp[i][2]) for i in hit], trellis=False)
            for i, p in zip(hit, paths):
                it, K, L = grp[i][:3]
                assert bits(p["score"]) == int(g["alt_bits"][it]), (path_mode, it, K, L)
                assert _same_steps(p, _golden_path(g, it)), (path_mode, it, K, L)
                walked += 1
    finally:
        engine.set_xtrans_table(np.zeros((0, 13), np.float32))
    assert walked >= 150


def test_long_profile_paths_are_the_references(engine, orc, path_mode):
    """large_classes.npz: every kernel class above one wavefront (K = 257 .. 16383, the strip class's row replay
    included), windows of <= 64 nt, 3 kb and 10 kb."""
    g = np.load(os.path.join(GOLDEN, "large_classes.npz"))
    cases = large_cases()
    assert len(cases) == len(g["K"]) == 32
    walked = 0
    for c in cases:
        i = c["idx"]
        want = _golden_path(g, i)
        if len(want[0]) == 0:  # no finite path
            continue
        prof, seq, xt = build_case(c, orc)
        engine.clear_profiles()
        engine.add_profile(prof.K, prof.trans, prof.match, prof.null, prof.bg)
        engine.commit()
        engine.set_sequences([seq])
        engine.set_mode(bool(c["mh"]), bool(c["h3"]))
        s = max(c["L"] // 3, 1)
        if c["quant"]:
            table = np.zeros((s + 1, 13), np.float32)
            table[s] = xt
            engine.set_xtrans_table(table)
        try:
            p = engine.path([(0, 0, 0, c["L"])], trellis=False)[0]
        finally:
            if c["quant"]:
                engine.set_xtrans_table(np.zeros((0, 13), np.float32))
        assert bits(p["score"]) == int(g["alt_bits"][i]), (path_mode, c)
        assert _same_steps(p, want), (path_mode, c)
        walked += 1
    assert walked >= 20


def test_minifam_paths_are_the_references(engine, path_mode):
    """minifam.dcp x the consensus reads x the four modes: every window that hits (minifam_consensus.npz)."""
    import deciphon_amd

    g = np.load(os.path.join(GOLDEN, "minifam_consensus.npz"))
    engine.clear_profiles()
    engine.load_dcp(os.path.join(GOLDEN, "minifam.dcp"))
    engine.commit()
    named = read_fasta(os.path.join(GOLDEN, "consensus.fna")) + read_fasta(os.path.join(GOLDEN, "consensus_multi.fna"))
    reads = [deciphon_amd.encode(s) for _, s in named]
    engine.set_sequences(reads)
    walked = 0
    for mh, h3 in MODES:
        engine.set_mode(bool(mh), bool(h3))
        sel = [j for j in np.nonzero((g["multi_hits"] == mh) & (g["hmmer3_compat"] == h3))[0]
               if len(_golden_path(g, j)[0])]
        wins = [(int(g["profile"][j]), int(g["read"][j]), 0, len(reads[int(g["read"][j])])) for j in sel]
        for j, w, p in zip(sel, wins, engine.path(wins, trellis=False)):
            assert bits(p["score"]) == int(g["alt_bits"][j]), (path_mode, mh, h3, w)
            assert _same_steps(p, _golden_path(g, j)), (path_mode, mh, h3, w)
            walked += 1
    assert walked >= 30


def _reference_table(orc, mh, h3):
    """rows 0 .. XT_ROWS of the reference's xtrans.c (row 0 unused): from oracle/_ref where it was built, else the
    oracle's rows once their SHA-256 is the one the reference's table has (reference_walks.npz)."""
    w = np.load(os.path.join(GOLDEN, "reference_walks.npz"))
    m = [tuple(int(v) for v in r) for r in w["xt_modes"]].index((mh, h3))
    ref = walks_reflib()
    xtrans = ref.xtrans if ref is not None else orc.xtrans
    rows = np.stack([xtrans(s, mh, h3) for s in range(1, XT_ROWS + 1)])
    assert hashlib.sha256(rows.tobytes()).hexdigest() == str(w["xt_sha256"][m])
    return np.concatenate([np.zeros((1, 13), np.float32), rows])


@pytest.mark.parametrize("mh,h3", [(1, 0), (0, 1)])
def test_xt_rows_of_every_kernel_family_are_the_references(engine, orc, mh, h3):
    """The cost kernels read the special transitions at row max(L / 3, 1) of the engine's table (DcpProblem.xt_row,
    DcpPack.xt_row).  Scores with the engine's own table equal, bit for bit, those with the reference's xtrans.c
    table handed over, for windows of every length 1 .. 600 and at 2 999 .. 3 001, 99 999 and 100 000 nt, on one
    profile per kernel family: pack (K = 40), one wave (200), narrow (300), multi-wave (1000), strip (4200); and on the
    short windows of the small profiles they are the oracle's with the reference's row."""
    rng = np.random.default_rng(600 + 2 * mh + h3)
    Ks = (40, 200, 300, 1000, 4200)
    profs = [synth_profile(rng, K) for K in Ks]
    read = random_seq(rng, 100000)
    engine.clear_profiles()
    for p in profs:
        engine.add_profile(p.K, p.trans, p.match, p.null, p.bg)
    engine.commit()
    engine.set_sequences([read])
    engine.set_mode(bool(mh), bool(h3))
    lengths = list(range(1, 601)) + [2999, 3000, 3001, 99999, 100000]
    wins = [(pi, 0, 0, L) for pi in range(len(Ks)) for L in lengths]
    table = _reference_table(orc, mh, h3)
    try:
        engine.set_xtrans_table(np.zeros((0, 13), np.float32))
        nul0, alt0 = engine.cost(wins)
        engine.set_xtrans_table(table)
        nul1, alt1 = engine.cost(wins)
    finally:
        engine.set_xtrans_table(np.zeros((0, 13), np.float32))
    assert np.isfinite(alt0).all()
    for i, w in enumerate(wins):
        assert bits(nul0[i]) == bits(nul1[i]) and bits(alt0[i]) == bits(alt1[i]), (Ks[w[0]], w[3])
    for i, (pi, _, a, b) in enumerate(wins):
        if Ks[pi] <= 300 and (b <= 64 or b % 97 == 0):
            xt = table[max(b // 3, 1)]
            assert bits(alt0[i]) == bits(orc.cost(profs[pi], xt, read[a:b])), (Ks[pi], b)
            assert bits(nul0[i]) == bits(orc.null(profs[pi], xt, read[a:b])), (Ks[pi], b)
