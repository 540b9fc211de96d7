"""CPU: the translation tables (host_logic.cpp: dcp_gencode_amino) and what press derives from them on the host
(hmm_model.cpp: dcp_setup_nuclt_dist) under every table the project holds, not only table 1.

The tables are held to tests/translation_tables.py, an independent statement of them.  The nucleotide distribution
and the 125 codon marginals of every entry (null, background, nodes 0..K) are held to a float64 model of codon_lprob,
nuclt_lprob (c-core/model.c) and imm_codon_marg written from their description: a codon weighs exp(log-odds of its
amino acid) / (codons of that amino acid), stops weigh 0, the weights are normalised over the 64 codons; p(b) is the
sum over codons of q * (occurrences of b) / 3; a marginal sums over its ANY positions.  The model is first held to the
reference itself -- tests/golden/minifam.dcp, pressed by the reference under table 1 -- within 1e-5 absolute, the
bound tests/test_press_host.py holds the library to on the same quantities; then the library is held to the model
within that bound under every table.

Worst |library - model| measured, minifam.hmm and the star profile together, per table (fp32 log-space sums against
float64): see DESIGN section 2 item 7."""
import os

import numpy as np
import pytest

import translation_tables as tt
from dcp_testlib import GOLDEN
from hmm_testlib import HMM, star_profile
from oracle.dcp_reader import read_dcp

DCP_EGENCODEID = 50
TOL = 1e-5
# HMMER3's Swiss-Prot 50.8 amino acid frequencies, in the order of its 20 columns (p7_AminoFrequencies)
SWISSPROT = (0.0787945, 0.0151600, 0.0535222, 0.0668298, 0.0397062, 0.0695071, 0.0229198, 0.0590092, 0.0594422,
             0.0963728, 0.0237718, 0.0414386, 0.0482904, 0.0395639, 0.0540978, 0.0683364, 0.0540687, 0.0673417,
             0.0114135, 0.0304133)
ANY = 4


# ---- the tables ---------------------------------------------------------------------------------------------

def test_the_statement_of_the_tables_is_consistent():
    assert tt.IDS == (1, 2, 3, 4, 5, 6, 9, 10, 11, 12)
    for gc in tt.IDS:
        t = tt.table(gc)
        assert len(t) == 64 and set(t.values()) == set(tt.AMINO) | {"*"}
        assert len(tt.stops(gc)) == tt.stop_count(gc)
        assert all(tt.table(1)[c] != aa for c, aa in tt.reassigned(gc).items())
    assert tt.stops(1) == ("TAA", "TAG", "TGA") and tt.stops(6) == ("TGA",)
    assert set(tt.stops(2)) == {"AGA", "AGG", "TAA", "TAG"}
    assert not set(tt.IDS) & set(tt.UNKNOWN_IDS)


@pytest.mark.parametrize("gc", tt.IDS)
def test_gencode_amino_equals_the_statement(gc):
    from deciphon_amd import host

    want = tt.table(gc)
    got = {codon: host.gencode_amino(gc, tt.indices(codon)) for codon in tt.CODONS}
    assert got == want, {c: (got[c], want[c]) for c in tt.CODONS if got[c] != want[c]}
    assert sum(aa == "*" for aa in got.values()) == tt.stop_count(gc)


def test_the_oracle_decoder_reads_the_same_tables():
    from oracle import pydecode

    for gc in tt.IDS:
        for codon in tt.CODONS:
            assert pydecode.gencode_amino(gc, tt.indices(codon)) == tt.table(gc)[codon], (gc, codon)


@pytest.mark.parametrize("gc", tt.UNKNOWN_IDS)
def test_tables_not_held_are_refused(gc, tmp_path):
    """NCBI defines 13-16 and 21-33 and the reference's schema lists them; this project holds none of them."""
    from deciphon_amd import DeciphonError, HipError, Press, host
    from deciphon_amd.host import HmmFile
    from deciphon_amd.scan import Scan

    for codon in ((0, 0, 0), (3, 2, 0), (0, 3, 2)):
        assert host.gencode_amino(gc, codon) == ""
    with pytest.raises(HipError) as e:
        HmmFile(HMM, gc)
    assert e.value.code == DCP_EGENCODEID
    with pytest.raises(DeciphonError) as e:
        Press(HMM, str(tmp_path / "x.dcp"), gencode=gc)
    assert e.value.code == DCP_EGENCODEID
    with pytest.raises(DeciphonError) as e:
        Scan.from_hmm(HMM, gencode=gc)
    assert e.value.code == DCP_EGENCODEID
    assert os.listdir(tmp_path) == []


# ---- the float64 model of codon_lprob, nuclt_lprob and the codon marginals ----------------------------------

def model_dist(gc, lodds):
    """lodds float64[entries, 20] (-inf = an amino acid of probability 0) -> (p[entries, 4], M[entries, 5, 5, 5]),
    probabilities, under translation table gc."""
    lodds = np.atleast_2d(np.asarray(lodds, np.float64))
    aminos = tt.aminos(gc)  # 64, in 3-mer code order
    w = np.zeros((len(lodds), 64))
    for c, aa in enumerate(aminos):
        if aa != "*":
            w[:, c] = np.exp(lodds[:, tt.AMINO.index(aa)]) / aminos.count(aa)
    q = (w / w.sum(axis=1, keepdims=True)).reshape(-1, 4, 4, 4)
    p = np.zeros((len(lodds), 4))
    for b in range(4):
        p[:, b] = (q[:, b].sum(axis=(1, 2)) + q[:, :, b].sum(axis=(1, 2)) + q[:, :, :, b].sum(axis=(1, 2))) / 3
    M = np.zeros((len(lodds), 5, 5, 5))
    M[:, :4, :4, :4] = q
    M[:, ANY, :4, :4] = q.sum(axis=1)
    M[:, :4, ANY, :4] = q.sum(axis=2)
    M[:, :4, :4, ANY] = q.sum(axis=3)
    M[:, ANY, ANY, :4] = q.sum(axis=(1, 2))
    M[:, ANY, :4, ANY] = q.sum(axis=(1, 3))
    M[:, :4, ANY, ANY] = q.sum(axis=(2, 3))
    M[:, ANY, ANY, ANY] = q.sum(axis=(1, 2, 3))
    return p, M


def null_lprobs():
    """the null model's amino acid log-probabilities: the frequencies narrowed to fp32 first (init_null_lprobs)"""
    return np.log(np.array(SWISSPROT, np.float32).astype(np.float64))


def profile_lodds(nodes):
    """The match lines of a profile's nodes, as text -> lodds[K + 3, 20]: entry 0 the null model (its own
    log-probabilities), 1 the background (zeros), 2 + n node n (its match log-probability, a fp32 value, minus the
    null's); entry 2 + K repeats node K - 1, as the end of a pressed profile does."""
    K = len(nodes)
    out = np.zeros((K + 3, 20))
    out[0] = null_lprobs()
    for k, nd in enumerate(nodes):
        match = np.array([-np.inf if v == "*" else np.float32(-float(v)) for v in nd["match"]], np.float64)
        out[2 + k] = match - null_lprobs()
    out[2 + K] = out[1 + K]
    return out


def deviation(got_nucltp, got_codonm, p, M, where):
    """The largest |got - log(model)| over both arrays; -inf exactly where the model is 0."""
    worst = 0.0
    for got, want in ((got_nucltp, p), (got_codonm, M.reshape(len(M), 125))):
        got = np.asarray(got, np.float64)
        assert got.shape == want.shape, where
        zero = want == 0.0
        assert not np.isnan(got).any() and not np.isposinf(got).any(), where
        assert np.array_equal(np.isneginf(got), zero), f"{where}: -inf where the model is not 0, or the reverse"
        worst = max(worst, float(np.abs(got[~zero] - np.log(want[~zero])).max()))
    return worst


def test_the_model_reproduces_the_reference_database():
    """The model itself, on table 1, against what the reference pressed: every nucltp and codonm of minifam.dcp."""
    from deciphon_amd import synth

    seeds = synth.load_hmm_seeds(HMM)
    db = read_dcp(os.path.join(GOLDEN, "minifam.dcp"))
    assert len(seeds) == len(db.proteins) == 3
    worst = 0.0
    for s, g in zip(seeds, db.proteins):
        assert g.gencode == 1 and len(s["nodes"]) == g.core_size
        p, M = model_dist(1, profile_lodds(s["nodes"]))
        assert np.isneginf(g.codonm).sum() == 3 * len(g.codonm)  # TAA, TAG and TGA of every entry
        worst = max(worst, deviation(g.nucltp, g.codonm, p, M, g.accession))
    print(f"model against the reference's minifam.dcp: worst deviation {worst:.3g}")
    assert worst <= TOL


@pytest.fixture(scope="module")
def profiles(tmp_path_factory):
    """(path, [node lists]) of minifam.hmm and of a file holding the 60-node star profile"""
    from deciphon_amd import synth

    seeds = synth.load_hmm_seeds(HMM)
    star = star_profile(seeds, np.random.default_rng(5))
    path = str(tmp_path_factory.mktemp("tables") / "star.hmm")
    synth.write_hmm(path, [star])
    return [(HMM, [s["nodes"] for s in seeds]), (path, [star["nodes"]])]


@pytest.mark.parametrize("gc", tt.IDS)
def test_host_distributions_equal_the_model_under_every_table(profiles, gc):
    from deciphon_amd.host import HmmFile

    worst, entries, zeros = 0.0, 0, 0
    for path, node_lists in profiles:
        with HmmFile(path, gc) as h:
            read = list(h)
        assert len(read) == len(node_lists)
        for got, nodes in zip(read, node_lists):
            K = got["core_size"]
            assert K == len(nodes) and got["nucltp"].shape == (K + 3, 4) and got["codonm"].shape == (K + 3, 125)
            p, M = model_dist(gc, profile_lodds(nodes))
            where = f"table {gc}, {got['accession']}"
            worst = max(worst, deviation(got["nucltp"], got["codonm"], p, M, where))
            # the library's own figures are distributions
            assert np.abs(np.exp(got["nucltp"].astype(np.float64)).sum(axis=1) - 1).max() <= TOL, where
            assert np.abs(np.exp(got["codonm"][:, 124].astype(np.float64)) - 1).max() <= TOL, where
            # every stop codon of this table is impossible in every entry; a codon it took from the stops is not
            codonm = got["codonm"].reshape(K + 3, 5, 5, 5)
            for codon in tt.stops(gc):
                assert np.isneginf(codonm[(slice(None),) + tt.indices(codon)]).all(), (where, codon)
            for codon in set(tt.stops(1)) - set(tt.stops(gc)):
                assert np.isfinite(codonm[:2][(slice(None),) + tt.indices(codon)]).all(), (where, codon)
            entries += K + 3
            zeros += int((M.reshape(K + 3, 125) == 0).sum()) - (K + 3) * tt.stop_count(gc)
    print(f"table {gc}: worst deviation from the float64 model {worst:.3g} over {entries} entries")
    assert worst <= TOL
    assert zeros > 0  # the star profile: marginals of whole amino acids at 0, beyond the stop codons
