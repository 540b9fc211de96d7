"""GPU: the cost-order copy of the emission rows (include/deciphon_host.h dcp_cost_order_map), made for the profiles
whose default cost kernel is (5,1) or (10,1).  Profiles of the classes of 384, 512 and 768 columns on both sides of
every boundary, some with delete runs that cost almost nothing, scored with the copy (the default), without it
(DECIPHON_HIP_COST_ORDER=0, read at ingest) and with the wide kernels on narrow profiles on top of either
(DECIPHON_HIP_NARROW=0: the kernel's shape is not the copy's, so it reads the canonical rows).  Every score must be
the oracle's, bit for bit; with the canonical match columns poisoned the narrow kernels must still score right (they
read the copy) and the wide ones must not; the path pass and a whole scan must not tell the layouts apart."""
import os

import numpy as np
import pytest

from dcp_testlib import GOLDEN, bits, random_seq, synth_profile

pytestmark = pytest.mark.gpu

KS = (257, 300, 320, 321, 384, 385, 448, 449, 512, 513, 600, 640, 641, 679, 768)
CHEAP_DELETES = {300, 385, 513, 641, 768}


def _profiles():
    rng = np.random.default_rng(404)
    out = []
    for K in KS:
        p = synth_profile(rng, K)
        if K in CHEAP_DELETES:  # delete runs across lanes and waves: the lazy D->D loop and the exchange
            a = K // 5
            p.trans[7, a : a + K // 2] = np.float32(0.01)  # DD
            p.trans[3, a] = np.float32(0.02)  # MD
        out.append(p)
    return out


@pytest.fixture(scope="module")
def cases(orc):
    rng = np.random.default_rng(405)
    profs = _profiles()
    reads = [random_seq(rng, n) for n in (97, 250, 413)]
    want = {}
    for i, p in enumerate(profs):
        for j, r in enumerate(reads):
            xt = orc.xtrans(max(len(r) // 3, 1), True, False)
            want[i, j] = (bits(orc.null(p, xt, r)), bits(orc.cost(p, xt, r)))
    return profs, reads, want


def _scores(profs, reads, monkeypatch, order, narrow: bool):
    import deciphon_amd

    monkeypatch.setenv("DECIPHON_HIP_COST_ORDER", order if isinstance(order, str) else "1" if order else "0")
    monkeypatch.setenv("DECIPHON_HIP_NARROW", "1" if narrow else "0")
    with deciphon_amd.Engine(0) as eng:
        for p in profs:
            eng.add_profile(p.K, p.trans, p.match, p.null, p.bg)
        eng.commit()
        eng.set_sequences(reads)
        eng.set_mode(True, False)
        wins = [(i, j, 0, len(r)) for i in range(len(profs)) for j, r in enumerate(reads)]
        nul, alt = eng.cost(wins)
        pool = eng.pool_bytes
    got = {(w[0], w[1]): (bits(nul[n]), bits(alt[n])) for n, w in enumerate(wins)}
    return got, pool


@pytest.mark.parametrize("order", [True, False], ids=["copy", "canonical"])
@pytest.mark.parametrize("narrow", [True, False], ids=["narrow", "wide"])
def test_scores_against_oracle(cases, monkeypatch, order, narrow):
    profs, reads, want = cases
    got, _ = _scores(profs, reads, monkeypatch, order, narrow)
    bad = [(profs[i].K, j) for (i, j), v in got.items() if v != want[i, j]]
    assert not bad, bad


COPIED = {K for K in KS if 257 <= K <= 320 or 513 <= K <= 640}  # default kernel (5,1) / (10,1)


def test_narrow_kernels_read_the_copy(cases, monkeypatch):
    """DECIPHON_HIP_COST_ORDER=poison zeroes the canonical match columns of the profiles that get a copy: the narrow
    kernels still give the oracle's bits there (they read the copy), the wide kernels on the same tables do not."""
    profs, reads, want = cases
    got, _ = _scores(profs, reads, monkeypatch, "poison", True)
    bad = [(profs[i].K, j) for (i, j), v in got.items() if v != want[i, j]]
    assert not bad, bad
    wide, _ = _scores(profs, reads, monkeypatch, "poison", False)
    for i, p in enumerate(profs):
        off = [wide[i, j][1] != want[i, j][1] for j in range(len(reads))]
        assert all(off) if p.K in COPIED else not any(off), p.K


def test_copy_costs_pool_bytes(cases, monkeypatch):
    profs, reads, _ = cases
    _, with_copy = _scores(profs, reads, monkeypatch, True, True)
    _, without = _scores(profs, reads, monkeypatch, False, True)
    assert without < with_copy < 2 * without


def test_path_pass_beside_copies(orc, monkeypatch):
    """The fast path pass (checkpoints every 40 rows; its kernels run the class shape and read the canonical rows)
    against the oracle's path, for profiles with and without a copy."""
    import deciphon_amd

    monkeypatch.setenv("DECIPHON_HIP_CKPT_ROWS", "40")
    monkeypatch.delenv("DECIPHON_HIP_COST_ORDER", raising=False)
    rng = np.random.default_rng(406)
    profs = [p for p in _profiles() if p.K in (300, 384, 449, 513, 641, 768)]
    read = random_seq(rng, 330)
    xt = orc.xtrans(max(len(read) // 3, 1), True, False)
    with deciphon_amd.Engine(0) as eng:
        for p in profs:
            eng.add_profile(p.K, p.trans, p.match, p.null, p.bg)
        eng.commit()
        eng.set_sequences([read])
        eng.set_mode(True, False)
        wins = [(i, 0, 0, len(read)) for i in range(len(profs))]
        paths = eng.path(wins)
    for p, got in zip(profs, paths):
        score, xo, no = orc.path(p, xt, read)
        assert bits(got["score"]) == bits(score), p.K
        assert np.array_equal(got["xnodes"], xo) and np.array_equal(got["nodes"], no), p.K


def test_scan_products_do_not_depend_on_the_layout(tmp_path, monkeypatch):
    from deciphon_amd import synth
    from test_gpu_scan import run_scan

    seeds = synth.load_seeds(os.path.join(GOLDEN, "minifam.dcp"))
    proteins = synth.pfam_like_database(seeds, len(KS), 91, lengths=np.array(KS))
    dcp = str(tmp_path / "cost_order.dcp")
    synth.write_dcp(dcp, proteins)
    rng = np.random.default_rng(407)
    reads = []
    for r, picks in enumerate(((1, 4, 9), (6, 11, 14))):
        x = rng.integers(0, 4, size=4000).astype(np.uint8)
        for j, pi in enumerate(picks):
            cons = proteins[pi]["consensus"]
            dom = synth.mutate(synth.back_translate(cons[:250]), rng, 0.08, 0.02, 0.02)
            x[200 + 1250 * j : 200 + 1250 * j + len(dom)] = dom
        reads.append((r + 1, "".join("ACGT"[v] for v in x)))
    rows = {}
    for order in ("1", "0"):
        monkeypatch.setenv("DECIPHON_HIP_COST_ORDER", order)
        d = tmp_path / f"out{order}"
        d.mkdir()
        rows[order] = run_scan(d, reads, dbfile=dcp)
    assert len(rows["1"]) >= 3
    assert rows["1"] == rows["0"]
