"""GPU: press, the pool and the kernels under every translation table the project holds, not only table 1.

One small synthetic .hmm (K = 1, 3, 40, 173 and a 60-node profile with * match emissions) is pressed under each of
the ten tables at epsilon = 0.01 and 0.  The pressed file's nucleotide distributions and codon marginals are those of
the host reader bit for bit -- tests/test_translation_tables.py holds them to a float64 model under every table -- and
every emission entry is held to dcp_testlib.emission_probs fed with them.  At epsilon = 0 the 3-mer of a stop codon of
the table is impossible in every row, and one the table took from the stops is not.  load_hmm leaves the pool of
press + load_dcp under every table; the kernels score a window with an in-frame TAA under table 6 and refuse it under
table 1; and scans under tables 1, 2, 4, 6 and 12 write the rows of the oracle scan, amino column included, on reads
whose planted domain is spelt with the codons those tables reassign."""
import numpy as np
import pytest

import dcp_testlib
import translation_tables as tt
from dcp_testlib import bits
from hmm_testlib import HMM, from_file, from_hmm, press, same_pools, star_profile, without_stops

pytestmark = pytest.mark.gpu

KS = (1, 3, 40, 173)  # and the star profile, K = 60
STAR = len(KS)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """The .hmm, and its pressed file per (table, error rate), pressed when first asked for."""
    from deciphon_amd import synth

    d = tmp_path_factory.mktemp("tables")
    seeds = synth.load_hmm_seeds(HMM)
    profiles = list(synth.pfam_like_hmms(seeds, len(KS), 71, lengths=list(KS)))
    profiles.append(star_profile(seeds, np.random.default_rng(5)))
    hmm = str(d / "tables.hmm")
    synth.write_hmm(hmm, profiles)
    pressed = {}

    def dcp(gc, epsilon):
        if (gc, epsilon) not in pressed:
            pressed[gc, epsilon] = press(hmm, str(d / f"t{gc}_{epsilon}.dcp"), gc, epsilon)
        return pressed[gc, epsilon]

    return hmm, dcp


# ---- press ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("epsilon", [0.01, 0.0])
@pytest.mark.parametrize("gc", tt.IDS)
def test_press_under_every_table(files, gc, epsilon):
    from deciphon_amd.host import Database, HmmFile

    hmm, dcp = files
    e32 = np.float32(epsilon)
    db = Database(dcp(gc, float(e32)))
    with HmmFile(hmm, gc) as h:
        read = list(h)
    assert len(db) == len(read) == len(KS) + 1 and db.epsilon == e32
    stop_codes = [20 + tt.code(c) for c in tt.stops(gc)]
    freed_codes = [20 + tt.code(c) for c in set(tt.stops(1)) - set(tt.stops(gc))]  # stops of table 1 that code here
    for i, host in enumerate(read):
        p = db.protein(i)
        K = p["core_size"]
        where = f"table {gc}, protein {i} (K = {K}) at epsilon {e32!r}"
        assert p["gencode"] == gc and K == host["core_size"] == (KS + (60,))[i], where
        for name in ("nucltp", "codonm"):
            assert np.array_equal(p[name].view(np.uint32), host[name].view(np.uint32)), (where, name)
        got = np.concatenate([p["null_emission"][None], p["bg_emission"][None], p["emission"]]).astype(np.float64)
        assert got.shape == (K + 3, 1364)
        want = dcp_testlib.emission_probs(float(e32), p["nucltp"], p["codonm"])
        zero = want == 0.0
        assert not np.isnan(got).any() and not np.isposinf(got).any(), where
        wrong_inf = np.isneginf(got) != zero
        assert not wrong_inf.any(), (f"{where}: {int(wrong_inf.sum())} entries -inf where the model is not 0 or the "
                                     f"reverse, first (row, code) {tuple(int(v) for v in np.argwhere(wrong_inf)[0])}")
        lw = np.log(want[~zero])
        err = np.abs(got[~zero] - lw) / np.maximum(1.0, np.abs(lw))
        worst = int(np.argmax(err))
        assert err[worst] <= 2e-5, f"{where}: relative log error {err[worst]:.3g} at log P = {lw[worst]:.6g}"
        if epsilon == 0.0:
            # said with the independent table: a stop codon of this table is impossible in every row (null, background
            # and every node), and a codon the table took from the stops is possible in every row -- but for those
            # nodes of the star profile that give its amino acid probability 0 (W under 2, 3, 4, 5 and 9: the nodes
            # k with k % 5 in {0, 1, 4}, and node K, the copy of K - 1)
            assert np.isneginf(got[:, stop_codes]).all(), where
            possible = np.ones(K + 3, bool)
            if i == STAR and gc in (2, 3, 4, 5, 9):
                k = np.minimum(np.arange(K + 1), K - 1)
                possible[2:] = ~np.isin(k % 5, (0, 1, 4))
            assert np.array_equal(np.isfinite(got[:, freed_codes]), np.repeat(possible[:, None], len(freed_codes), 1)), where
    db.close()


# ---- the pool ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def pool_of_table_1(files):
    hmm, dcp = files
    return from_file(dcp(1, 0.01))


@pytest.mark.parametrize("gc", tt.IDS)
def test_load_hmm_leaves_the_pool_of_the_pressed_file(files, pool_of_table_1, gc):
    hmm, dcp = files
    a = from_file(dcp(gc, 0.01)) if gc != 1 else pool_of_table_1
    b = from_hmm(hmm, gc, 0.01)
    assert [K for K, _, _ in b] == list(KS) + [60]
    same_pools(a, b)
    for (K, _, w), (_, _, w1) in zip(b, pool_of_table_1):  # and it is this table's pool: another one than table 1's
        assert np.array_equal(w, w1) == (gc in (1, 11)), (gc, K)


# ---- the kernels at epsilon = 0: what is a stop decides what can be scored ------------------------------------

def test_in_frame_taa_scores_under_table_6_and_not_under_table_1(files, orc):
    import deciphon_amd
    from oracle.dcp_reader import read_dcp

    hmm, dcp = files
    L = 300
    x = np.random.default_rng(6).integers(0, 4, size=L).astype(np.uint8)
    for at in (30, 150, 291):
        x[at : at + 3] = tt.indices("TAA")
    x = without_stops(x, tt.stops(6))
    text = "".join("ACGT"[v] for v in x)
    assert "TGA" not in text and all(text[at : at + 3] == "TAA" for at in (30, 150, 291))
    wins = [(i, 0, 0, L) for i in range(len(KS) + 1)]
    scores = {}
    for gc in (6, 1):
        with deciphon_amd.Engine(0) as eng:
            eng.load_dcp(dcp(gc, 0.0))
            eng.commit()
            eng.set_sequences([x])
            eng.set_mode(True, False)
            scores[gc] = eng.cost(wins)
    proteins = read_dcp(dcp(6, 0.0)).proteins
    xt = orc.xtrans(L // 3, True, False)
    for i, p in enumerate(proteins):
        prof = orc.setup_profile(p)
        want_nul, want_alt = orc.null(prof, xt, x), orc.cost(prof, xt, x)
        assert np.isfinite(want_nul) and np.isfinite(want_alt), p.core_size
        assert bits(scores[6][0][i]) == bits(want_nul) and bits(scores[6][1][i]) == bits(want_alt), p.core_size
        assert bits(scores[1][0][i]) == bits(np.inf) and bits(scores[1][1][i]) == bits(np.inf), p.core_size


# ---- scans ------------------------------------------------------------------------------------------------

# table -> the amino acid planted at every fourth node, and the codons it is spelt with in the read: the ones the
# table reassigns (table 1, the control: W has the one codon)
PLANT = {1: ("W", ("TGG",)), 2: ("W", ("TGA",)), 4: ("W", ("TGA",)), 6: ("Q", ("TAA", "TAG")), 12: ("S", ("CTG",))}
SCAN_KS = (40, 173)  # a pack shape; one wavefront
READ = 600


def planted_profiles(gc):
    """Two profiles whose every fourth node has PLANT[gc]'s amino acid as its consensus residue.  Every node emits
    its consensus residue with probability 0.9: sharp enough that the read is a hit under table 1 too, where a
    quarter of its codons are stops or spell another amino acid, so that the two match columns can be compared."""
    from deciphon_amd import synth

    profiles = list(synth.pfam_like_hmms(synth.load_hmm_seeds(HMM), len(SCAN_KS), 83, lengths=list(SCAN_KS)))
    for p in profiles:
        for k, nd in enumerate(p["nodes"]):
            aa = PLANT[gc][0] if k % 4 == 0 else nd["tail"][1].upper()
            assert aa in tt.AMINO
            nd["match"] = ["0.10536" if a == aa else "5.24702" for a in tt.AMINO]  # 0.9, and 0.1 / 19 each
            nd["tail"] = [nd["tail"][0], aa] + list(nd["tail"][2:])
    return profiles


def planted_reads(gc, profiles):
    """One read of 600 nt per profile: its consensus back-translated, every fourth residue with the codons of
    PLANT[gc], then mutated lightly (2 % substitutions, 0.5 % insertions and deletions)."""
    from deciphon_amd import synth

    aa, codons = PLANT[gc]
    reads = []
    for i, p in enumerate(profiles):
        rng = np.random.default_rng([gc, i, 9])
        cons = [nd["tail"][1].upper() for nd in p["nodes"]]
        assert all(c == aa for c in cons[::4])
        text = "".join(codons[(k // 4) % len(codons)] if k % 4 == 0 else synth.CODON.get(a, "GCT")
                       for k, a in enumerate(cons))
        dom = synth.mutate(np.array([tt.NUCLT.index(ch) for ch in text], np.uint8), rng, 0.02, 0.005, 0.005)
        x = rng.integers(0, 4, size=READ).astype(np.uint8)
        assert len(dom) <= READ - 40
        x[30 : 30 + len(dom)] = dom
        reads.append((i + 1, "".join(tt.NUCLT[v] for v in x)))
    return reads


def planted_cells(rows, gc):
    """{accession: cells of the rows' match columns that decode to a codon of PLANT[gc] with its amino acid}"""
    aa, codons = PLANT[gc]
    n = {}
    for row in rows:
        f = row.split("\t")
        cells = [c.split(",") for c in f[11].split(";")]
        n[f[7]] = n.get(f[7], 0) + sum(1 for c in cells if c[2] in codons and c[3] == aa)
    return n


@pytest.mark.parametrize("gc", sorted(PLANT))
def test_scan_rows_equal_the_oracle_scan_under_the_table(tmp_path, orc, gc):
    from deciphon_amd import synth
    from deciphon_amd.scan import Batch, Scan, Sequence
    from oracle.dcp_reader import read_dcp

    profiles = planted_profiles(gc)
    reads = planted_reads(gc, profiles)
    hmm = str(tmp_path / "planted.hmm")
    synth.write_hmm(hmm, profiles)
    dcp = press(hmm, str(tmp_path / "planted.dcp"), gc, 0.01)
    proteins = read_dcp(dcp).proteins
    assert [p.gencode for p in proteins] == [gc, gc] and [p.core_size for p in proteins] == list(SCAN_KS)
    # the oracle first: the test is about reassigned codons only if its rows hold them
    want = dcp_testlib.oracle_scan(orc, proteins, reads, True, False, epsilon=0.01, gencode=gc)
    planted = planted_cells(want, gc)
    assert sorted(planted) == sorted(p.accession for p in proteins)
    assert all(n >= 5 for n in planted.values()), planted

    batch = Batch()
    for sid, text in reads:
        batch.add(Sequence(sid, f"r{sid}", text))
    with Scan(dcp, 0, 1, True, False, False) as scan:
        scan.run(str(tmp_path / "pressed"), batch)
        rows = scan.products()
    with Scan.from_hmm(hmm, gc, 0.01) as scan:
        scan.run(str(tmp_path / "direct"), batch)
        direct = scan.products()
    assert rows == want
    assert direct == want
    assert open(tmp_path / "direct" / "products.tsv").read() == open(tmp_path / "pressed" / "products.tsv").read()
    if gc != 1:
        # Table 1 reads the same reads differently: the oracle's rows under table 1, none of whose cells reads a codon
        # that way and none of whose match columns is one of the above.  Under table 12 both profiles are still hit
        # (CTG spells L).  Under 2, 4 and 6 a quarter of the domain's codons are stops of table 1, and the oracle
        # finds no hit at all: no input with a reassigned stop at every fourth residue is a hit under table 1.
        dcp1 = press(hmm, str(tmp_path / "planted1.dcp"), 1, 0.01)
        with Scan(dcp1, 0, 1, True, False, False) as scan:
            scan.run(str(tmp_path / "table1"), batch)
            rows1 = scan.products()
        assert rows1 == dcp_testlib.oracle_scan(orc, read_dcp(dcp1).proteins, reads, True, False, epsilon=0.01)
        if gc == 12:
            assert sorted(planted_cells(rows1, gc)) == sorted(planted)
        assert sum(planted_cells(rows1, gc).values()) == 0
        assert not set(r.split("\t")[11] for r in rows1) & set(r.split("\t")[11] for r in rows)
