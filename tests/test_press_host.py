"""CPU: the host half of press -- the HMMER3 reader and the protein model (csrc/hmm_model.cpp) -- against the
reference's own pressed database.  tests/golden/minifam.dcp was pressed by the reference from
tests/golden/minifam.hmm (c-core/minifam.hmm), so every field press computes on the host is pinned by it:
accession, consensus and K equal, transitions bit for bit, nucleotide distributions, codon marginals and the
occupancy entry within 1e-5 (fp32 rounding of imm's log-space arithmetic, whose source is not in the tree)."""
import os

import numpy as np
import pytest

from dcp_testlib import GOLDEN
from oracle.dcp_reader import read_dcp

HMM = os.path.join(GOLDEN, "minifam.hmm")
DCP_EFOPEN, DCP_EFUNCUSE, DCP_EZEROMODEL, DCP_ELARGEMODEL, DCP_EREADHMMER3 = 33, 8, 12, 15, 17
DCP_ELONGACCESSION, DCP_EGENCODEID, DCP_EENDOFFILE, DCP_EENDOFNODES = 41, 50, 66, 67


def close_with_inf(got, want, tol=1e-5):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    inf = np.isinf(want)
    assert np.array_equal(np.isinf(got), inf)
    assert np.array_equal(got[inf], want[inf])
    return float(np.abs(got[~inf] - want[~inf]).max()) <= tol


def read_all(path, gencode=1):
    from deciphon_amd.host import HmmFile

    with HmmFile(path, gencode) as h:
        return len(h), list(h)


def test_minifam_model_equals_the_reference_database():
    n, profiles = read_all(HMM)
    db = read_dcp(os.path.join(GOLDEN, "minifam.dcp"))
    assert n == len(profiles) == len(db.proteins) == 3
    for p, g in zip(profiles, db.proteins):
        K = g.core_size
        assert (p["accession"], p["consensus"], p["core_size"]) == (g.accession, g.consensus, K)
        assert p["has_ga"] is True
        assert p["trans"].shape == (K + 1, 7)
        assert np.array_equal(p["trans"].view(np.uint32), g.trans.view(np.uint32))  # -inf and -0.0 included
        assert close_with_inf(p["BMk"], g.BMk)
        # entries 0 (null), 1 (background) and 2 + n for every node n = 0..K
        assert close_with_inf(p["nucltp"], g.nucltp)
        assert close_with_inf(p["codonm"], g.codonm)
    assert db.header["has_ga"] is True


def test_massive_parses():
    n, profiles = read_all(os.path.join(GOLDEN, "massive.hmm"))
    assert n == 1 and len(profiles) == 1
    p = profiles[0]
    assert (p["accession"], p["core_size"], len(p["consensus"])) == ("PF01073.21", 3, 3)
    assert np.isfinite(p["BMk"]).all() and np.isfinite(p["nucltp"]).all()


def test_other_translation_tables_and_unknown_ones():
    from deciphon_amd import HipError

    _, std = read_all(HMM, 1)
    _, t11 = read_all(HMM, 11)  # the same amino table as 1 (only start codons differ)
    assert np.array_equal(std[0]["codonm"], t11[0]["codonm"])
    _, t4 = read_all(HMM, 4)  # TGA codes W: one stop fewer
    TGA = 3 * 25 + 2 * 5 + 0
    assert np.isinf(std[0]["codonm"][2:, TGA]).all() and np.isfinite(t4[0]["codonm"][2:, TGA]).all()
    with pytest.raises(HipError) as e:
        read_all(HMM, 999)
    assert e.value.code == DCP_EGENCODEID


def _profile0_text():
    text = open(HMM).read()
    return text[: text.index("//\n") + 3]


def _rc(tmp_path, text):
    from deciphon_amd import HipError

    path = tmp_path / "bad.hmm"
    path.write_text(text)
    try:
        read_all(str(path))
    except HipError as e:
        return e.code
    return 0


def test_malformed_inputs_give_the_reference_error_codes(tmp_path):
    good = _profile0_text()
    assert _rc(tmp_path, good) == 0
    lines = good.splitlines(keepends=True)
    node2 = next(i for i, ln in enumerate(lines) if ln.split()[:1] == ["2"])
    # a node line cut short
    cut = lines[:node2] + [" ".join(lines[node2].split()[:12]) + "\n"] + lines[node2 + 1 :]
    assert _rc(tmp_path, "".join(cut)) == DCP_EENDOFNODES
    # the file ends inside the nodes: no `//`
    assert _rc(tmp_path, good[: -len("//\n")]) == DCP_EENDOFNODES
    # LENG says more nodes than there are, or fewer
    assert _rc(tmp_path, good.replace("LENG  173", "LENG  174")) == DCP_EENDOFNODES
    assert _rc(tmp_path, good.replace("LENG  173", "LENG  172")) == DCP_ELARGEMODEL
    # accessions of 32 bytes do not fit struct protein's accession[32]; 31 do
    assert _rc(tmp_path, good.replace("PF00742.20", "A" * 32)) == DCP_ELONGACCESSION
    assert _rc(tmp_path, good.replace("PF00742.20", "A" * 31)) == 0
    # MODEL_MAX = 16384 (c-core/model.h:12), and an empty model
    assert _rc(tmp_path, good.replace("LENG  173", "LENG  16385")) == DCP_ELARGEMODEL
    assert _rc(tmp_path, good.replace("LENG  173", "LENG  0")) == DCP_EZEROMODEL
    # not a HMMER3/f file; no LENG; a value that is not a number; the file ends after the header
    assert _rc(tmp_path, "HMMER2.0\n" + good) == DCP_EREADHMMER3
    assert _rc(tmp_path, good.replace("LENG  173\n", "")) == DCP_EREADHMMER3
    compo = next(i for i, ln in enumerate(lines) if ln.split()[:1] == ["COMPO"])
    assert _rc(tmp_path, "".join(lines[: compo + 2] + [lines[compo + 2].replace("0.03203", "x")] + lines[compo + 3 :])) \
        == DCP_EREADHMMER3
    assert _rc(tmp_path, "".join(lines[:compo])) == DCP_EENDOFFILE
    # a second profile's error comes after the first profile is read
    from deciphon_amd.host import HmmFile

    (tmp_path / "two.hmm").write_text(good + good.replace("LENG  173", "LENG  0"))
    with HmmFile(str(tmp_path / "two.hmm")) as h:
        assert len(h) == 2
        assert h.next()["core_size"] == 173
        with pytest.raises(Exception) as e:
            h.next()
        assert e.value.code == DCP_EZEROMODEL


def test_missing_file():
    from deciphon_amd import HipError

    with pytest.raises(HipError) as e:
        read_all("/nonexistent/minifam.hmm")
    assert e.value.code == DCP_EFOPEN


def test_press_without_a_usable_gpu_creates_nothing(tmp_path, monkeypatch):
    """No gfx950 at DECIPHON_HIP_DEVICE: open fails with DCP_EFUNCUSE before the output exists.  Where a GPU is
    present, the device index is pointed past the last one, which is the same refusal."""
    import deciphon_amd
    from deciphon_amd import DeciphonError, Press

    monkeypatch.setenv("DECIPHON_HIP_DEVICE", str(deciphon_amd.device_count()))
    out = tmp_path / "minifam.dcp"
    press = Press(HMM, str(out), 1, 0.01)
    with pytest.raises(DeciphonError) as e:
        press.open()
    assert e.value.code == DCP_EFUNCUSE
    assert os.listdir(tmp_path) == []
    assert press.nproteins == 0 and not press.end()
    press.close()  # nothing is open: a no-op


def test_press_call_order_and_setup_errors(tmp_path):
    from deciphon_amd import DeciphonError, Press

    press = Press(HMM, str(tmp_path / "x.dcp"))
    with pytest.raises(DeciphonError) as e:
        press.next()  # before open
    assert e.value.code == DCP_EFUNCUSE
    with pytest.raises(DeciphonError) as e:
        Press(HMM, str(tmp_path / "x.dcp"), gencode=999)
    assert e.value.code == DCP_EGENCODEID
    for eps in (-0.1, 1.5, float("nan")):
        with pytest.raises(DeciphonError) as e:
            Press(HMM, str(tmp_path / "x.dcp"), epsilon=eps)
        assert e.value.code == DCP_EFUNCUSE
    assert os.listdir(tmp_path) == []


def test_synthetic_hmm_writer_round_trips():
    """deciphon_amd.synth writes HMMER3 text from resampled minifam nodes; minifam's own profile 0 rewritten by it
    reads back identically."""
    from deciphon_amd import synth

    seeds = synth.load_hmm_seeds(HMM)
    assert [len(s["nodes"]) for s in seeds] == [173, 241, 162]
    import tempfile

    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "rt.hmm")
        synth.write_hmm(path, [dict(accession="PF00742.20", name="Homoserine_dh", compo=seeds[0]["compo"],
                                    nodes=seeds[0]["nodes"])])
        _, (a,) = read_all(path)
        b = read_all(HMM)[1][0]
        for k in ("trans", "BMk", "nucltp", "codonm"):
            assert np.array_equal(a[k], b[k]), k
        assert a["consensus"] == b["consensus"]
        path = os.path.join(d, "syn.hmm")
        assert synth.write_hmm(path, synth.pfam_like_hmms(seeds, 4, 7, lengths=[1, 2, 300, 5000])) == 4
        n, ps = read_all(path)
        assert n == 4 and [p["core_size"] for p in ps] == [1, 2, 300, 5000]
        assert all(np.isfinite(p["BMk"]).all() for p in ps)
