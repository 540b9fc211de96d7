"""The reads of the both-strand scan tests and what the CPU oracle says of them (tests/test_gpu_strands.py)."""
import os

import numpy as np

import dcp_testlib
from dcp_testlib import GOLDEN, read_fasta

DCP = os.path.join(GOLDEN, "minifam.dcp")
HMM = os.path.join(GOLDEN, "minifam.hmm")
HEADER13 = ["sequence", "window", "window_start", "window_stop", "hit", "hit_start", "hit_stop", "profile", "abc", "lrt",
            "evalue", "match", "strand"]


def rc_text(text: str) -> str:
    """The reverse complement of an unambiguous DNA or RNA text (A<->T or A<->U, C<->G)."""
    comp = {"A": "U" if "U" in text else "T", "C": "G", "G": "C", "T": "A", "U": "A"}
    return "".join(comp[c] for c in reversed(text))


def rc_nt(x) -> np.ndarray:
    return (3 - np.asarray(x, np.uint8)[::-1]).astype(np.uint8)


def consensus():
    return [t for _, t in read_fasta(os.path.join(GOLDEN, "consensus.fna"))]


def scan_reads():
    """[(id, text)]: a read as its profile has it, one reversed, one with a domain on either strand, and a long one with
    five planted domains, three of them on the minus strand, whose chains have more than one window."""
    cons = consensus()
    long = ["ACGT"[i] for i in np.random.default_rng(31).integers(0, 4, 20000)]
    for at, dom in ((1500, cons[0]), (6000, rc_text(cons[0])), (9000, cons[1]), (13000, rc_text(cons[2])),
                    (16500, rc_text(cons[1]))):
        long[at : at + len(dom)] = dom
    return [(1, cons[0]), (2, rc_text(cons[1])), (3, cons[2] + "ACGTTGCA" * 5 + rc_text(cons[0])), (4, "".join(long))]


def merge_strands(plus_rows, minus_rows, proteins, reads):
    """Rows of plain scans of the reads and of their reverse complements -> the rows of a scan of both strands: a
    strand column, and (profile, read, strand with + first, window) order."""
    prof = {p.accession: i for i, p in enumerate(proteins)}
    read = {str(sid): i for i, (sid, _) in enumerate(reads)}
    rows = [r + "\t+" for r in plus_rows] + [r + "\t-" for r in minus_rows]

    def key(r):
        f = r.split("\t")
        return prof[f[7]], read[f[0]], f[12] == "-", int(f[1])

    return sorted(rows, key=key)


def oracle_both(orc, proteins, reads, rc=rc_text, **kw):
    """(rows of both strands, plus rows, minus rows): dcp_testlib.oracle_scan of the reads and of their reverse
    complements, which is all the oracle knows of strands."""
    threads = min(os.cpu_count() or 1, 16)
    plus = dcp_testlib.oracle_scan(orc, proteins, reads, True, False, threads=threads, **kw)
    minus = dcp_testlib.oracle_scan(orc, proteins, [(sid, rc(t)) for sid, t in reads], True, False, threads=threads, **kw)
    return merge_strands(plus, minus, proteins, reads), plus, minus
