"""GPU: dcp_press_* end to end -- HMMER3 text in, .dcp out, emission tables from press_kernel.hip.

Pinned by the reference's own pressed database (tests/golden/minifam.dcp, pressed from tests/golden/minifam.hmm):
every field within the bounds of tests/test_press_host.py, every emission entry within 2e-5 max(1, |x|) (the bound
tests/test_decoder.py uses), the header equal, and a scan of the pressed file giving the reference's products.tsv.
Beyond minifam the kernel is checked against the quasi-codon model (oracle/pydecode.py) in float64, on synthetic
profiles from K = 1 to MODEL_MAX and three error rates."""
import glob
import itertools
import os

import numpy as np
import pytest

import dcp_testlib
from dcp_testlib import GOLDEN, read_fasta
from oracle import pydecode
from oracle.dcp_reader import read_dcp

pytestmark = pytest.mark.gpu

HMM = os.path.join(GOLDEN, "minifam.hmm")
CODE_OFF = (0, 4, 20, 84, 340)
CODES = [(CODE_OFF[n - 1] + i, list(z)) for n in range(1, 6) for i, z in enumerate(itertools.product(range(4), repeat=n))]
DCP_EFOPEN, DCP_EFUNCUSE, DCP_EZEROMODEL, DCP_EGENCODEID = 33, 8, 12, 50


def press(hmm, out, gencode=1, epsilon=0.01):
    from deciphon_amd import Press

    with Press(hmm, out, gencode, epsilon) as p:
        n = p.nproteins
        calls = 0
        while not p.end():
            p.next()
            calls += 1
    assert calls == n + 1  # one protein per next, end() true after the call that found none
    assert not [f for f in os.listdir(os.path.dirname(out)) if f.startswith(os.path.basename(out) + ".")]
    return n


def close_with_inf(got, want, tol):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    inf = np.isinf(want)
    assert np.array_equal(np.isinf(got), inf)
    assert np.array_equal(got[inf], want[inf])
    d = np.abs(got[~inf] - want[~inf])
    return bool((d <= tol * np.maximum(1.0, np.abs(want[~inf]))).all())


def test_press_minifam_matches_reference_database(tmp_path):
    from deciphon_amd.host import Database

    out = str(tmp_path / "minifam.dcp")
    assert press(HMM, out) == 3
    gold = read_dcp(os.path.join(GOLDEN, "minifam.dcp"))
    got = read_dcp(out)
    for k in ("magic_number", "version", "entry_dist", "epsilon", "abc", "amino", "has_ga"):
        assert got.header[k] == gold.header[k], k
    assert len(got.proteins) == len(got.protein_sizes) == 3
    db = Database(out)
    assert len(db) == 3 and db.entry_dist == 2 and db.has_ga and db.epsilon == np.float32(0.01)
    for i, (p, g) in enumerate(zip(got.proteins, gold.proteins)):
        assert (p.accession, p.gencode, p.consensus, p.core_size) == (g.accession, g.gencode, g.consensus, g.core_size)
        assert np.array_equal(p.trans.view(np.uint32), g.trans.view(np.uint32))
        assert close_with_inf(p.BMk, g.BMk, 1e-5)
        assert close_with_inf(p.nucltp, g.nucltp, 1e-5)
        assert close_with_inf(p.codonm, g.codonm, 1e-5)
        for table in ("emission", "null_emission", "bg_emission"):
            assert close_with_inf(getattr(p, table), getattr(g, table), 2e-5), (i, table)
        # the product's own reader sees the same
        q = db.protein(i)
        assert q["accession"] == p.accession and np.array_equal(q["emission"], p.emission)
        assert np.array_equal(q["nucltp"], p.nucltp) and np.array_equal(q["trans"], p.trans)
    db.close()


def test_pressed_minifam_scan_reproduces_reference_products(tmp_path):
    from deciphon_amd.scan import Batch, Scan, Sequence

    out = str(tmp_path / "minifam.dcp")
    press(HMM, out)
    batch = Batch()
    for i, (_, s) in enumerate(read_fasta(os.path.join(GOLDEN, "consensus.fna"))):
        batch.add(Sequence(i, f"seq{i}", s))
    prod = tmp_path / "prod"
    with Scan(out, 0, 1, True, False, False) as scan:
        scan.run(str(prod), batch)
        rows = scan.products()
    gold = [ln.rstrip("\n").split("\t") for ln in open(os.path.join(GOLDEN, "products.tsv"))][1:]
    assert len(rows) == len(gold) == 3
    for got, want in zip(rows, gold):
        g = got.split("\t")
        assert g[:10] == want[:10]
        assert g[11] == want[11]


@pytest.fixture(scope="module")
def synthetic_hmm(tmp_path_factory):
    from deciphon_amd import synth

    path = str(tmp_path_factory.mktemp("press") / "synthetic.hmm")
    seeds = synth.load_hmm_seeds(HMM)
    synth.write_hmm(path, synth.pfam_like_hmms(seeds, 7, 11, lengths=[1, 2, 3, 173, 641, 4097, 16384]))
    return path


@pytest.mark.parametrize("epsilon", [0.0, 0.01, 0.1])
def test_kernel_equals_the_model_on_synthetic_profiles(synthetic_hmm, tmp_path, epsilon):
    from deciphon_amd.host import Database

    out = str(tmp_path / "synthetic.dcp")
    assert press(synthetic_hmm, out, 1, epsilon) == 7
    db = Database(out)
    assert db.epsilon == np.float32(epsilon)
    e = float(np.float32(epsilon))
    for i in range(len(db)):
        p = db.protein(i)
        K = p["core_size"]
        checks = [(0, p["null_emission"]), (1, p["bg_emission"])] if i == 0 else []
        checks += [(2 + n, p["emission"][n]) for n in sorted({0, K // 2, K - 1, K})]
        for entry, table in checks:
            pr = np.exp(p["nucltp"][entry].astype(np.float64))
            M = np.exp(p["codonm"][entry].astype(np.float64)).reshape(5, 5, 5)
            for code, z in CODES:
                want = pydecode.emission_prob(e, pr, M, z)
                got = float(table[code])
                if epsilon == 0.0 and len(z) != 3:
                    assert got == -np.inf, (K, entry, z)
                elif want == 0.0:
                    assert got == -np.inf, (K, entry, z)
                else:
                    lw = np.log(want)
                    assert abs(got - lw) <= 2e-5 * max(1.0, abs(lw)), (K, entry, z, got, lw)
    db.close()


def test_presses_are_deterministic_and_independent_of_batching(tmp_path, monkeypatch):
    from deciphon_amd import synth
    from deciphon_amd.host import Database

    seeds = synth.load_hmm_seeds(HMM)
    profiles = list(synth.pfam_like_hmms(seeds, 9, 5, lengths=[40, 250, 90, 700, 5, 310, 128, 64, 1000]))
    profiles[3]["ga"] = False
    multi = str(tmp_path / "multi.hmm")
    synth.write_hmm(multi, profiles)
    a, b = str(tmp_path / "a.dcp"), str(tmp_path / "b.dcp")
    press(multi, a)
    press(multi, b)
    assert open(a, "rb").read() == open(b, "rb").read()
    # batches of at most 300 nodes: read-ahead boundaries fall between and after most profiles
    monkeypatch.setenv("DECIPHON_HIP_PRESS_BATCH_NODES", "300")
    c = str(tmp_path / "c.dcp")
    press(multi, c)
    assert open(c, "rb").read() == open(a, "rb").read()
    whole = open(a, "rb").read()
    db = Database(a)
    assert not db.has_ga  # the AND over proteins
    for i, p in enumerate(profiles):
        one_hmm, one_dcp = str(tmp_path / f"one{i}.hmm"), str(tmp_path / f"one{i}.dcp")
        synth.write_hmm(one_hmm, [p])
        press(one_hmm, one_dcp)
        one = Database(one_dcp)
        lo, hi = one.offset(0), os.path.getsize(one_dcp)
        assert whole[db.offset(i) : db.offset(i) + hi - lo] == open(one_dcp, "rb").read()[lo:hi], i
        one.close()
    db.close()


def test_massive_pressed_and_scanned_equals_the_oracle(tmp_path, orc):
    """massive.hmm (K = 3) pressed, then every window of the chain of one 10 kb read scored on the GPU: null and
    alt scores equal the CPU oracle's bit for bit, given the pressed tables; dcp_scan_run's rows equal the
    oracle scan's."""
    import deciphon_amd
    from deciphon_amd import host
    from deciphon_amd.scan import Batch, Scan, Sequence

    out = str(tmp_path / "massive.dcp")
    assert press(os.path.join(GOLDEN, "massive.hmm"), out) == 1
    db = read_dcp(out)
    assert db.proteins[0].core_size == 3
    rng = np.random.default_rng(3)
    read = "".join(rng.choice(list("ACGT"), size=10000))
    nt = deciphon_amd.encode(read)
    prof = orc.setup_profile(db.proteins[0])
    wins = []
    it = host.WindowIter(len(nt), 3)
    while (w := it.next()) is not None:
        wins.append((0, 0, w[1], w[2]))
    assert len(wins) > 70
    with deciphon_amd.Engine(0) as eng:
        eng.load_dcp(out)
        eng.commit()
        eng.set_sequences([nt])
        eng.set_mode(True, False)
        nul, alt = eng.cost(wins)
    for i, (_, _, a, b) in enumerate(wins):
        seq = np.ascontiguousarray(nt[a:b])
        xt = orc.xtrans(max((b - a) // 3, 1), True, False)
        assert dcp_testlib.bits(nul[i]) == dcp_testlib.bits(orc.null(prof, xt, seq)), i
        assert dcp_testlib.bits(alt[i]) == dcp_testlib.bits(orc.cost(prof, xt, seq)), i
    batch = Batch()
    batch.add(Sequence(1, "seq1", read))
    with Scan(out, 0, 1, True, False, False) as scan:
        scan.run(str(tmp_path / "prod"), batch)
        rows = scan.products()
    assert rows == dcp_testlib.oracle_scan(orc, db.proteins, [(1, read)], True, False)


def test_error_paths(tmp_path):
    from deciphon_amd import DeciphonError, Press

    with pytest.raises(DeciphonError) as e:
        Press(HMM, str(tmp_path / "x.dcp"), gencode=77)
    assert e.value.code == DCP_EGENCODEID
    # a missing .hmm; an output directory that cannot be written (a path through a regular file)
    with pytest.raises(DeciphonError) as e:
        Press(str(tmp_path / "missing.hmm"), str(tmp_path / "x.dcp")).open()
    assert e.value.code == DCP_EFOPEN
    (tmp_path / "file").write_text("")
    with pytest.raises(DeciphonError) as e:
        Press(HMM, str(tmp_path / "file" / "x.dcp")).open()
    assert e.value.code == DCP_EFOPEN
    assert sorted(os.listdir(tmp_path)) == ["file"]
    # next after end
    p = Press(HMM, str(tmp_path / "m.dcp"))
    p.open()
    while not p.end():
        p.next()
    with pytest.raises(DeciphonError) as e:
        p.next()
    assert e.value.code == DCP_EFUNCUSE
    p.close()
    assert sorted(os.listdir(tmp_path)) == ["file", "m.dcp"]
    # the third profile is malformed: two proteins are pressed, the third next fails, close leaves nothing
    good = open(HMM).read()
    first = good[: good.index("//\n") + 3]
    (tmp_path / "bad.hmm").write_text(first + first + first.replace("LENG  173", "LENG  0") + first)
    p = Press(str(tmp_path / "bad.hmm"), str(tmp_path / "bad.dcp"))
    p.open()
    assert p.nproteins == 4
    p.next()
    p.next()
    with pytest.raises(DeciphonError) as e:
        p.next()
    assert e.value.code == DCP_EZEROMODEL
    with pytest.raises(DeciphonError) as e:
        p.next()
    assert e.value.code == DCP_EFUNCUSE
    p.close()
    assert sorted(os.listdir(tmp_path)) == ["bad.hmm", "file", "m.dcp"]
    assert not glob.glob(str(tmp_path / "*.dcp.*"))
