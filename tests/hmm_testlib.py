"""Shared helpers of the tests that press, load and scan HMMER3 files: pressing to the end, synthetic .hmm files,
the pool of an engine as words, and reads without stop codons."""
from __future__ import annotations

import os

import numpy as np

from dcp_testlib import GOLDEN

HMM = os.path.join(GOLDEN, "minifam.hmm")


def press(hmm, out, gencode=1, epsilon=0.01):
    from deciphon_amd import Press

    with Press(hmm, out, gencode, epsilon) as p:
        while not p.end():
            p.next()
    return out


def synthetic_hmm(path, lengths, seed):
    from deciphon_amd import synth

    seeds = synth.load_hmm_seeds(HMM)
    assert synth.write_hmm(path, synth.pfam_like_hmms(seeds, len(lengths), seed, lengths=list(lengths))) == len(lengths)
    return path


def star_profile(seeds, rng, K=60, accession="STAR0.1"):
    """A profile with zero-probability (*) match emissions -- every (2 + k % 5)-th amino acid of node k -- so that
    codon marginals of whole amino acids are 0."""
    from deciphon_amd import synth

    star = synth.resample_hmm(seeds, K, rng, accession)
    for k, nd in enumerate(star["nodes"]):
        nd["match"] = [("*" if j % (2 + k % 5) == 0 else v) for j, v in enumerate(nd["match"])]
    return star


AMINO = "ACDEFGHIKLMNPQRSTVWY"  # the order of a HMMER3 match line
# the nodes of edge_profile, in order; (amino acid, nats) = almost one-hot: every other amino acid that far down
EDGE_NODES = ("real0", "real1", "real2", "star", ("M", 60), ("M", 200), ("L", 60), ("L", 200), "uniform")


def edge_profile(seeds, rng, accession="EDGE0.1"):
    """One node per kind of match emission the emission kernels can meet (EDGE_NODES): three as a real profile has
    them, one of star_profile's (half the amino acids at probability 0), almost one-hot ones for an amino acid of one
    codon (M) and of six (L) with every other amino acid at e^-60 and at e^-200 of it -- at 200 a product of three
    inputs, e^-600, is still a normal double --, and a uniform one."""
    from deciphon_amd import synth

    prof = synth.resample_hmm(seeds, len(EDGE_NODES), rng, accession)
    star = star_profile(seeds, rng, K=4)["nodes"][0]["match"]
    for nd, kind in zip(prof["nodes"], EDGE_NODES):
        if kind == "star":
            nd["match"] = list(star)
        elif kind == "uniform":
            nd["match"] = ["2.99573"] * 20
        elif isinstance(kind, tuple):
            nd["match"] = ["0.00000" if a == kind[0] else f"{kind[1]:.5f}" for a in AMINO]
    return prof


def pool_words(eng, first=0, last=None):
    """(K, accession, words) of profiles [first, last) as they lie in the pool."""
    last = eng.num_profiles if last is None else last
    return [(eng.core_size(i), eng.accession(i), eng.profile_tables(i).view(np.uint32)) for i in range(first, last)]


def same_pools(a, b):
    assert len(a) == len(b)
    for (Ka, acc_a, wa), (Kb, acc_b, wb) in zip(a, b):
        assert (Ka, acc_a) == (Kb, acc_b)
        assert wa.shape == wb.shape, Ka
        if not np.array_equal(wa, wb):
            at = np.flatnonzero(wa != wb)
            raise AssertionError(f"K={Ka}: {len(at)} of {len(wa)} words differ, first at {at[:8]}")


def from_file(dcp, **kw):
    import deciphon_amd

    with deciphon_amd.Engine(0) as eng:
        eng.load_dcp(dcp, **kw)
        return pool_words(eng)


def from_hmm(hmm, *args, **kw):
    import deciphon_amd

    with deciphon_amd.Engine(0) as eng:
        eng.load_hmm(hmm, *args, **kw)
        return pool_words(eng)


def without_stops(x, stops=("TAA", "TAG", "TGA")):
    """x with the first nucleotide of every stop codon, in any frame, turned into one that leaves no stop in the three
    codons it is part of: at epsilon = 0 a window whose length is a multiple of 3 then has finite null and alt
    scores.  `stops` are the table's (translation_tables.stops); C is tried first, and no table held has a stop with
    a C in it, so under table 1 this is: the T of every TAA, TAG and TGA becomes a C."""
    stop = {tuple("ACGT".index(ch) for ch in s) for s in stops}
    x = np.array(x, np.uint8)

    def stop_at(j):
        return (int(x[j]), int(x[j + 1]), int(x[j + 2])) in stop

    for i in range(len(x) - 2):
        if not stop_at(i):
            continue
        for v in (1, 0, 2, 3):
            x[i] = v
            if not any(stop_at(j) for j in range(max(i - 2, 0), i + 1)):
                break
        else:
            raise ValueError(f"no nucleotide at {i} leaves the codons around it free of stops")
    return x
