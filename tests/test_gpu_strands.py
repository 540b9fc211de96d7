"""GPU: both strands of every read (dcp_hip_set_sequences_strands, dcp_scan_set_strands; the kernels of csrc/code_rows.hip).

The minus strand exists only as code rows that the GPU writes from the one upload of the reads.  So: those rows, word
for word, against the host statement (dcp_code_rows_of); the cost and path passes over a minus-strand window against the
same window of the explicitly reverse-complemented read, bit for bit; and the scan's file against the CPU oracle's scan
of the reads and of their reverse complements, merged into (profile, read, strand, window) order."""
import os

import numpy as np
import pytest

import deciphon_amd
import strands_cases as sc
from deciphon_amd import hit_on_read, host
from dcp_testlib import bits, random_seq, synth_profile
from oracle.dcp_reader import read_dcp

pytestmark = pytest.mark.gpu

EFUNCUSE, ESEQABC = 8, 57
LENGTHS = list(range(12)) + [255, 256, 257, 513]


def palindrome(n, rng):
    half = random_seq(rng, n // 2)
    return np.concatenate([half, sc.rc_nt(half)])


def check_rows(eng, reads):
    assert eng.num_sequences == 2 * len(reads)
    for s, x in enumerate(reads):
        assert np.array_equal(eng.code_rows(2 * s), host.code_rows_of(x)), (s, len(x), "+")
        assert np.array_equal(eng.code_rows(2 * s + 1), host.code_rows_of(x, minus=True)), (s, len(x), "-")


# ---- 1. the rows, word for word --------------------------------------------------------------------------------------

def test_rows_of_both_strands_word_for_word():
    rng = np.random.default_rng(5)
    reads = []
    for n in LENGTHS:
        reads += [random_seq(rng, n), np.zeros(n, np.uint8), np.full(n, 3, np.uint8)]
    reads += [palindrome(n, rng) for n in (2, 10, 256, 512)]
    with deciphon_amd.Engine(0) as eng:
        eng.set_sequences(reads, "both")
        check_rows(eng, reads)
        for s in range(len(reads) - 4, len(reads)):  # a reverse palindrome: minus rows are plus rows
            assert np.array_equal(eng.code_rows(2 * s), eng.code_rows(2 * s + 1))
        both_plus = [eng.code_rows(2 * s) for s in range(len(reads))]
        eng.set_sequences(reads)  # the plus rows are what a plain set_sequences leaves
        assert eng.num_sequences == len(reads)
        for s in range(len(reads)):
            assert np.array_equal(eng.code_rows(s), both_plus[s])
        eng.set_sequences(reads, "plus")
        assert eng.num_sequences == len(reads)
        assert np.array_equal(eng.code_rows(len(reads) - 1), both_plus[-1])


def test_rows_of_more_reads_than_grid_rows():
    """65 539 reads of length i mod 8: more sequences than gridDim.y holds, so the kernel strides over them."""
    rng = np.random.default_rng(6)
    n = 65539
    lens = np.arange(n) % 8
    nt = random_seq(rng, int(lens.sum()))
    off = np.concatenate([[0], np.cumsum(lens)])
    reads = [nt[off[i] : off[i + 1]] for i in range(n)]
    with deciphon_amd.Engine(0) as eng:
        eng.set_sequences(reads, "both")
        assert eng.num_sequences == 2 * n
        # the host statement once per distinct read (there are few: lengths 0..7), the device rows one by one
        want = {}
        for s, x in enumerate(reads):
            k = x.tobytes()
            if k not in want:
                want[k] = (host.code_rows_of(x), host.code_rows_of(x, minus=True))
            p, m = want[k]
            assert np.array_equal(eng.code_rows(2 * s), p), s
            assert np.array_equal(eng.code_rows(2 * s + 1), m), s
        eng.set_sequences(reads)  # and the plain kernel strides there as well
        assert eng.num_sequences == n
        for s, x in enumerate(reads):
            assert np.array_equal(eng.code_rows(s), want[x.tobytes()][0]), s


def test_rows_of_a_read_longer_than_the_grid():
    """A read of 262 151 rows, more than the 1024 blocks of 256 threads a grid has at the most in x: every kernel's loop
    over the rows takes a second turn, and the short reads ride in a grid sized by the long one."""
    rng = np.random.default_rng(9)
    long = 262150
    reads = [random_seq(rng, n) for n in (0, long, 1, 5)]
    seed, freq = 20262, [0.1, 0.2, 0.3, 0.4]
    with deciphon_amd.Engine(0) as eng:
        eng.set_sequences(reads, "plus")
        assert eng.num_sequences == len(reads)
        for s, x in enumerate(reads):
            assert np.array_equal(eng.code_rows(s), host.code_rows_of(x)), (s, "+")
        eng.set_sequences(reads, "both")
        check_rows(eng, reads)
        eng.set_random_sequences(2, long, seed, freq)
        assert eng.num_sequences == 2
        for s in range(2):
            assert np.array_equal(eng.code_rows(s), host.code_rows_of(host.random_nt(seed, long, s * long, freq))), s


def test_refusals_leave_the_previous_reads_in_force():
    rng = np.random.default_rng(7)
    first = [random_seq(rng, n) for n in (40, 7, 0, 129)]
    other = [random_seq(rng, n) for n in (33, 90)]
    prof = synth_profile(rng, 12)
    with deciphon_amd.Engine(0) as eng:
        eng.add_profile(prof.K, prof.trans, prof.match, prof.null, prof.bg)
        eng.commit()
        eng.set_mode(True, False)
        eng.set_sequences(first, "both")
        bad = [other[0], np.array([0, 1, 2, 3, 4], np.uint8)]
        with pytest.raises(deciphon_amd.HipError) as e:
            eng.set_sequences(bad, "both")
        assert e.value.code == ESEQABC
        check_rows(eng, first)
        for value in (2, -1):
            with pytest.raises(deciphon_amd.HipError) as e:
                eng.set_sequences(other, value)
            assert e.value.code == EFUNCUSE
            check_rows(eng, first)
        eng.cost_hits_begin([(0, 1, 0, 40), (0, 6, 0, 100)])
        try:
            for strands in ("both", "plus"):
                with pytest.raises(deciphon_amd.HipError) as e:
                    eng.set_sequences(other, strands)
                assert e.value.code == EFUNCUSE
            check_rows(eng, first)  # (a read-only query: allowed while the batch is outstanding)
        finally:
            eng.cost_hits_end()
        eng._seq_lens = [len(x) for x in first for _ in range(2)]  # (the wrapper's own note of the refused calls)
        check_rows(eng, first)
        eng.set_sequences(other, "both")
        check_rows(eng, other)


# ---- 2. the engine: a minus-strand window is the window of the reverse-complemented read ------------------------------

def test_cost_and_path_of_minus_windows_equal_those_of_reversed_reads():
    rng = np.random.default_rng(8)
    profs = [synth_profile(rng, K) for K in (12, 140, 700)]  # a pack shape, one wavefront, several
    reads = [random_seq(rng, 300) for _ in range(3)]
    spans = [(0, 300), (0, 120), (137, 300), (41, 263)]  # whole reads, a prefix, a suffix, an inner span
    with deciphon_amd.Engine(0) as both, deciphon_amd.Engine(0) as plain:
        for eng in (both, plain):
            for p in profs:
                eng.add_profile(p.K, p.trans, p.match, p.null, p.bg)
            eng.commit()
            eng.set_mode(True, False)
        both.set_sequences(reads, "both")
        plain.set_sequences([sc.rc_nt(x) for x in reads])
        wb = [(p, 2 * s + 1, a, b) for p in range(3) for s in range(3) for a, b in spans]
        wp = [(p, s, a, b) for p in range(3) for s in range(3) for a, b in spans]
        nb, ab = both.cost(wb)
        np_, ap = plain.cost(wp)
        pb, pp = both.path(wb, trellis=False), plain.path(wp, trellis=False)
        for i, w in enumerate(wb):
            assert bits(nb[i]) == bits(np_[i]) and bits(ab[i]) == bits(ap[i]), w
            assert bits(pb[i]["score"]) == bits(pp[i]["score"]), w
            assert np.array_equal(pb[i]["state_ids"], pp[i]["state_ids"]), w
            assert np.array_equal(pb[i]["seqsizes"], pp[i]["seqsizes"]), w
            assert len(pb[i]["state_ids"]) > 2, w
        # and the plus strand beside it is the read as given
        plain.set_sequences(reads)
        wq = [(p, 2 * s, a, b) for p, s, a, b in wp]
        nq, aq = both.cost(wq)
        nr, ar = plain.cost(wp)
        assert [bits(v) for v in nq] == [bits(v) for v in nr] and [bits(v) for v in aq] == [bits(v) for v in ar]
        assert [bits(v) for v in aq] != [bits(v) for v in ab]  # (the strands do differ)


# ---- 3. the scan against the oracle ------------------------------------------------------------------------------------

def run_scan(directory, reads, strands="both", dbfile=sc.DCP, scan=None, **kw):
    from deciphon_amd.scan import Batch, Scan, Sequence

    batch = Batch()
    for sid, text in reads:
        batch.add(Sequence(sid, f"seq{sid}", text))
    own = scan is None
    if own:
        scan = Scan(dbfile, 0, 1, True, False, False, strands=strands, **kw)
    try:
        scan.run(str(directory), batch)
        assert scan.progress() == 100
        rows = scan.products()
        mode = scan.strands
    finally:
        if own:
            scan.free()
    lines = open(os.path.join(str(directory), "products.tsv")).read().splitlines()
    assert lines[0].split("\t") == (sc.HEADER13 if mode == "both" else sc.HEADER13[:12])
    assert lines[1:] == rows
    return rows


@pytest.fixture(scope="module")
def expected(orc):
    """The oracle's rows of the reads and of their reverse complements, computed once."""
    reads = sc.scan_reads()
    both, plus, minus = sc.oracle_both(orc, read_dcp(sc.DCP).proteins, reads)
    return reads, both, plus, minus


def test_scan_of_both_strands_against_the_oracle(tmp_path, expected):
    reads, want, plus, minus = expected
    # (so that the test cannot pass on an empty strand: reads 3 and 4 hit on both, one minus row in window 1)
    assert (len(plus), len(minus)) == (4, 5)
    assert {r.split("\t")[0] for r in plus} & {r.split("\t")[0] for r in minus} == {"3", "4"}
    assert [r.split("\t")[1:4] for r in minus if r.split("\t")[1] != "0"] == [["1", "7959", "16609"]]
    rows = run_scan(tmp_path / "both", reads)
    assert rows == want
    assert all(len(r.split("\t")) == 13 for r in rows)
    # the hit of the reversed read 2 is the whole read, on the minus strand
    (r2,) = [r for r in rows if r.startswith("2\t")]
    assert hit_on_read(r2, len(reads[1][1])) == (0, 723, "-")
    # read 4: every planted domain where it was planted, on the strand it was planted on
    L4 = len(reads[3][1])
    assert sorted(hit_on_read(r, L4) for r in rows if r.startswith("4\t")) == [
        (1500, 2019, "+"), (6000, 6519, "-"), (9000, 9723, "+"), (13000, 13486, "-"), (16500, 17223, "-")]
    # nothing speculated: the same file
    os.environ["DECIPHON_HIP_SPECULATE"] = "0"
    try:
        assert run_scan(tmp_path / "rounds", reads) == rows
    finally:
        del os.environ["DECIPHON_HIP_SPECULATE"]
    # two partitions concatenate to the whole
    parts = []
    for idx in range(2):
        parts += run_scan(tmp_path / f"p{idx}", reads, partition=(0, idx, 2))
    assert parts == rows


def test_scan_from_hmm_and_back_to_the_plus_strand(tmp_path, expected):
    from deciphon_amd.press import Press
    from deciphon_amd.scan import Scan

    reads, _, plus, _ = expected
    pressed = str(tmp_path / "minifam.dcp")
    with Press(sc.HMM, pressed) as press:
        while not press.end():
            press.next()
    want = run_scan(tmp_path / "pressed", reads, dbfile=pressed)
    assert len(want) >= 9 and {r[-1] for r in want} == {"+", "-"}
    with Scan.from_hmm(sc.HMM, strands="both") as scan:
        assert scan.strands == "both"
        assert run_scan(tmp_path / "hmm", reads, scan=scan) == want
        scan.set_strands("plus")
        assert scan.strands == "plus"
        twelve = run_scan(tmp_path / "hmm_plus", reads, scan=scan)
    never = run_scan(tmp_path / "never", reads, strands="plus", dbfile=pressed)  # a scan that never heard of strands
    assert twelve == never == [r[:-2] for r in want if r.endswith("\t+")]
    assert all(len(r.split("\t")) == 12 for r in twelve)
    # and on the committed database, whose plus rows the oracle has
    with Scan(sc.DCP, strands="both") as scan:
        scan.set_strands("plus")
        assert run_scan(tmp_path / "dcp_plus", reads, scan=scan) == plus
        scan.set_strands("both")
        assert len(run_scan(tmp_path / "dcp_both", reads, scan=scan)) == 9


# ---- 4. what the minus strand is ---------------------------------------------------------------------------------------

def test_rna_read_prints_u_on_the_minus_strand(tmp_path):
    from deciphon_amd import synth

    cons = sc.consensus()
    dna = sc.rc_text(cons[1])
    rna = dna.replace("T", "U")
    assert "U" in rna and "T" not in rna
    rna_db = str(tmp_path / "minifam_rna.dcp")
    db = host.Database(sc.DCP)
    synth.write_dcp(rna_db, [db.protein(i) for i in range(len(db))], epsilon=db.epsilon, rna=True)
    db.close()
    got = run_scan(tmp_path / "rna", [(5, rna)], dbfile=rna_db)
    want = run_scan(tmp_path / "dna", [(5, dna)])
    assert len(got) == len(want) == 1 and want[0].endswith("\t-")

    def as_rna(row):
        f = row.split("\t")
        assert f[8] == "dna"
        f[8] = "rna"
        cells = []
        for cell in f[11].split(";"):
            nts, state, codon, amino = cell.split(",")  # (an amino acid may be T: only nucleotides change)
            cells.append(",".join([nts.replace("T", "U"), state, codon.replace("T", "U"), amino]))
        f[11] = ";".join(cells)
        return "\t".join(f)

    assert got[0] == as_rna(want[0])  # the steps of the DNA read, spelt with U
    match = got[0].split("\t")[11]
    assert "U" in match and not any("T" in c.split(",")[0] + c.split(",")[2] for c in match.split(";"))
    assert "".join(c.split(",")[0] for c in match.split(";")) == sc.rc_text(rna) == cons[1].replace("T", "U")


def iupac(text: str) -> str:
    t = list(text)
    for k, i in enumerate(range(49, len(t), 50)):
        t[i] = "NRY"[k % 3]
    return "".join(t)


def test_minus_strand_is_the_reverse_complement_of_the_disambiguated_read(tmp_path, orc):
    """Reads carrying IUPAC letters: a domain with N, R or Y for every 50th letter, and the same thing done to the
    domain's reverse complement, whose domain is then on the minus strand.  The minus strand is the reverse complement
    of what dcp_batch_add keeps of the read -- deciphon_amd.hip.encode spelt back as letters -- so the rows are the
    oracle's of those texts and of their reverse complements."""
    cons = sc.consensus()
    texts = [iupac(cons[0]), iupac(sc.rc_text(cons[0]))]
    kept = ["".join("ACGT"[i] for i in deciphon_amd.hip.encode(t)) for t in texts]
    assert all(k != t and len(k) == len(t) for k, t in zip(kept, texts))
    want, plus, minus = sc.oracle_both(orc, read_dcp(sc.DCP).proteins, [(1, kept[0]), (2, kept[1])])
    assert (len(plus), len(minus)) == (1, 1)  # the domain of read 1 on its plus strand, of read 2 on its minus strand
    rows = run_scan(tmp_path / "iupac", [(1, texts[0]), (2, texts[1])])
    assert [r for r in rows if r.endswith("\t-")] == [r for r in want if r.endswith("\t-")]
    assert rows == want

