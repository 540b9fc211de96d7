"""TEST INFRASTRUCTURE ONLY -- the NCBI translation tables the project holds, stated independently of
deciphon_amd/csrc/host_logic.cpp.

Table 1 (the standard code) is data: per amino acid, its codons.  Every other table is its documented differences
from table 1, as NCBI's "The Genetic Codes" describes them (which codons change meaning), not a 64-letter string:
a typing slip in host_logic.cpp's strings cannot repeat itself here by copying.  Nucleotides are the project's
indices A, C, G, T = 0..3; a codon's 3-mer code is 16 a + 4 b + c.
"""
from __future__ import annotations

import itertools

NUCLT = "ACGT"
AMINO = "ACDEFGHIKLMNPQRSTVWY"  # the order of HMMER's 20 columns

# the standard code: amino acid (or * = stop) -> its codons
STANDARD = {
    "A": "GCT GCC GCA GCG",
    "C": "TGT TGC",
    "D": "GAT GAC",
    "E": "GAA GAG",
    "F": "TTT TTC",
    "G": "GGT GGC GGA GGG",
    "H": "CAT CAC",
    "I": "ATT ATC ATA",
    "K": "AAA AAG",
    "L": "TTA TTG CTT CTC CTA CTG",
    "M": "ATG",
    "N": "AAT AAC",
    "P": "CCT CCC CCA CCG",
    "Q": "CAA CAG",
    "R": "CGT CGC CGA CGG AGA AGG",
    "S": "TCT TCC TCA TCG AGT AGC",
    "T": "ACT ACC ACA ACG",
    "V": "GTT GTC GTA GTG",
    "W": "TGG",
    "Y": "TAT TAC",
    "*": "TAA TAG TGA",
}

# id -> ({codon: amino acid} that differ from table 1, number of stop codons)
DIFFERENCES = {
    1: ({}, 3),
    2: ({"AGA": "*", "AGG": "*", "ATA": "M", "TGA": "W"}, 4),  # vertebrate mitochondrial
    3: ({"ATA": "M", "CTT": "T", "CTC": "T", "CTA": "T", "CTG": "T", "TGA": "W"}, 2),  # yeast mitochondrial
    4: ({"TGA": "W"}, 2),  # mold, protozoan, coelenterate mitochondrial; mycoplasma, spiroplasma
    5: ({"AGA": "S", "AGG": "S", "ATA": "M", "TGA": "W"}, 2),  # invertebrate mitochondrial
    6: ({"TAA": "Q", "TAG": "Q"}, 1),  # ciliate, dasycladacean and hexamita nuclear
    9: ({"AAA": "N", "AGA": "S", "AGG": "S", "TGA": "W"}, 2),  # echinoderm and flatworm mitochondrial
    10: ({"TGA": "C"}, 2),  # euplotid nuclear
    11: ({}, 3),  # bacterial, archaeal and plant plastid: the amino acids of table 1
    12: ({"CTG": "S"}, 3),  # alternative yeast nuclear
}
IDS = tuple(DIFFERENCES)
# ids the project does not hold; NCBI (and the reference's schema) define 13-16 and 21-33
UNKNOWN_IDS = (-1, 0, 7, 8, 13, 14, 15, 16) + tuple(range(21, 34)) + (77, 999)

CODONS = tuple("".join(c) for c in itertools.product(NUCLT, repeat=3))  # in 3-mer code order


def _standard():
    t = {codon: aa for aa, codons in STANDARD.items() for codon in codons.split()}
    assert sorted(t) == sorted(CODONS) and len(STANDARD) == 21
    return t


def table(gencode: int) -> dict:
    """{codon text: amino acid or '*'} of all 64 codons."""
    diff, _ = DIFFERENCES[gencode]
    t = _standard()
    assert all(t[c] != aa for c, aa in diff.items())  # every listed difference is one
    t.update(diff)
    return t


def indices(codon: str):
    return tuple(NUCLT.index(ch) for ch in codon)


def code(codon: str) -> int:
    a, b, c = indices(codon)
    return 16 * a + 4 * b + c


def amino(gencode: int, codon) -> str:
    """The amino acid of a codon given as text or as three nucleotide indices."""
    if not isinstance(codon, str):
        codon = "".join(NUCLT[int(v)] for v in codon)
    return table(gencode)[codon]


def aminos(gencode: int) -> str:
    """The 64 amino acids in 3-mer code order (AAA, AAC, ... TTT)."""
    t = table(gencode)
    return "".join(t[c] for c in CODONS)


def stops(gencode: int):
    """The stop codons, as text, in code order."""
    t = table(gencode)
    return tuple(c for c in CODONS if t[c] == "*")


def stop_count(gencode: int) -> int:
    return DIFFERENCES[gencode][1]


def reassigned(gencode: int) -> dict:
    """{codon: amino acid} of the codons that table 1 reads differently."""
    return dict(DIFFERENCES[gencode][0])
