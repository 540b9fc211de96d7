"""CPU: the host half of dcp_hip_set_gencode / dcp_scan_set_gencode -- the amino log-odds a profile keeps, the
recomputation of its nodes' distributions from them under another translation table (dcp_regencode_entries), the models
of a table without a file (dcp_hmm_models) -- and the argument checks that come before the device.

Everything is compared word for word with what the reader gives when the file is opened under the target table: the
recomputation is the reader's own function on the reader's own inputs, so there is no tolerance."""
import numpy as np
import pytest

import translation_tables as tt
from deciphon_amd import host
from hmm_testlib import HMM, star_profile, synthetic_hmm

DCP_EFUNCUSE, DCP_EGENCODEID = 8, 50
KS = (1, 3, 64, 65, 300)  # and the star profile, K = 60: match emissions of *, log-odds of -inf
# every ordered pair (s, t) of the two sweeps: from table 1 to all ten, and from all ten to table 1
PAIRS = [(1, t) for t in tt.IDS] + [(s, 1) for s in tt.IDS if s != 1]


def words(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def read_under(tmp_path_factory):
    """{file: per table the profiles as HmmFile reads them}, read when first asked for."""
    from deciphon_amd import synth

    d = tmp_path_factory.mktemp("set_gencode_host")
    seeds = synth.load_hmm_seeds(HMM)
    profiles = list(synth.pfam_like_hmms(seeds, len(KS), 91, lengths=list(KS)))
    profiles.append(star_profile(seeds, np.random.default_rng(92)))
    synthetic = str(d / "synthetic.hmm")
    assert synth.write_hmm(synthetic, profiles) == len(KS) + 1
    paths = {"minifam": HMM, "synthetic": synthetic}
    cache = {}

    def read(name, gc):
        if (name, gc) not in cache:
            with host.HmmFile(paths[name], gc) as h:
                cache[name, gc] = list(h)
        return cache[name, gc]

    return read


def entries_of(p):
    """The kept entries of a profile's K nodes as the load writes them: nucltp[4], codonm[125], three floats of 0."""
    K = p["core_size"]
    out = np.zeros((K, host.ENTRY_FLOATS), np.float32)
    out[:, :4] = p["nucltp"][2 : 2 + K]
    out[:, 4:129] = p["codonm"][2 : 2 + K]
    return out


@pytest.mark.parametrize("name", ["minifam", "synthetic"])
@pytest.mark.parametrize("s,t", PAIRS, ids=[f"{s}-to-{t}" for s, t in PAIRS])
def test_entries_from_lodds_are_the_readers_under_the_target_table(read_under, name, s, t):
    src, dst = read_under(name, s), read_under(name, t)
    assert len(src) == len(dst) >= 3
    if name == "synthetic":
        assert [p["core_size"] for p in src] == list(KS) + [60]
        assert np.isneginf(src[-1]["lodds"]).any()
    for a, b in zip(src, dst):
        assert a["lodds"].shape == (a["core_size"], 20)
        got = host.regencode_entries(t, a["lodds"])
        want = entries_of(b)
        assert got.shape == want.shape
        assert np.array_equal(words(got), words(want)), (name, a["accession"], s, t)
        # the padding floats are what the load writes: +0.0, the word 0
        assert (words(got)[:, 129:] == 0).all()


@pytest.mark.parametrize("name", ["minifam", "synthetic"])
def test_lodds_do_not_depend_on_the_table(read_under, name):
    first = read_under(name, 1)
    assert any(np.isfinite(p["lodds"]).all() for p in first)
    for gc in tt.IDS:
        for a, b in zip(first, read_under(name, gc)):
            assert np.array_equal(words(a["lodds"]), words(b["lodds"])), (name, gc, a["accession"])


def test_the_tables_give_different_entries(read_under):
    """Or the comparisons above would pass on a recomputation that ignored its table."""
    p = read_under("synthetic", 1)[4]
    seen = {gc: host.regencode_entries(gc, p["lodds"]).tobytes() for gc in tt.IDS}
    assert seen[1] == seen[11]  # the same code: they differ in their start codons only
    assert len(set(seen.values())) == len(tt.IDS) - 1


@pytest.mark.parametrize("gc", tt.IDS)
def test_models_of_a_table_without_a_file(read_under, gc):
    nucltp, codonm = host.hmm_models(gc)
    assert nucltp.shape == (2, 4) and codonm.shape == (2, 125)
    for name in ("minifam", "synthetic"):
        for p in read_under(name, gc):
            assert np.array_equal(words(nucltp), words(p["nucltp"][:2])), (name, gc)
            assert np.array_equal(words(codonm), words(p["codonm"][:2])), (name, gc)
    assert host.HmmFile.models(gc)[1].tobytes() == codonm.tobytes()
    # either output may be NULL
    L = host._lib()
    only = np.zeros((2, 125), np.float32)
    assert L.dcp_hmm_models(gc, None, only.ctypes.data) == 0 and only.tobytes() == codonm.tobytes()
    assert L.dcp_hmm_models(gc, None, None) == 0


def test_thread_caps_give_the_same_bytes(read_under):
    lodds = np.concatenate([p["lodds"] for p in read_under("synthetic", 1)])
    assert len(lodds) == sum(KS) + 60
    one = host.regencode_entries(4, lodds, 1)
    assert one.tobytes() == host.regencode_entries(4, lodds, 16).tobytes()
    # caps outside 1..16 are clamped, not refused
    assert one.tobytes() == host.regencode_entries(4, lodds, 0).tobytes()
    assert one.tobytes() == host.regencode_entries(4, lodds, 1000).tobytes()
    assert not np.isnan(one).any()  # every entry was written
    assert host.regencode_entries(4, np.zeros((0, 20), np.float32)).shape == (0, host.ENTRY_FLOATS)


@pytest.mark.parametrize("gc", [0, 7, 13, 34])
def test_a_table_not_held(gc):
    with pytest.raises(host.HipError) as e:
        host.regencode_entries(gc, np.zeros((2, 20), np.float32))
    assert e.value.code == DCP_EGENCODEID
    with pytest.raises(host.HipError) as e:
        host.hmm_models(gc)
    assert e.value.code == DCP_EGENCODEID


def test_regencode_entries_checks_its_arguments():
    L = host._lib()
    out = np.zeros(host.ENTRY_FLOATS, np.float32)
    lodds = np.zeros(20, np.float32)
    assert L.dcp_regencode_entries(1, -1, lodds.ctypes.data, 1, out.ctypes.data) == DCP_EFUNCUSE
    assert L.dcp_regencode_entries(1, 1, None, 1, out.ctypes.data) == DCP_EFUNCUSE
    assert L.dcp_regencode_entries(1, 1, lodds.ctypes.data, 1, None) == DCP_EFUNCUSE
    assert L.dcp_regencode_entries(1, 0, None, 1, None) == 0
    assert L.dcp_hmm_read_lodds(None, out.ctypes.data) == DCP_EFUNCUSE


def test_lodds_of_a_file_before_its_first_profile():
    L = host._lib()
    out = np.zeros(20, np.float32)
    with host.HmmFile(HMM) as h:
        assert L.dcp_hmm_read_lodds(h.h, out.ctypes.data) == DCP_EFUNCUSE
        assert h.next() is not None
        assert L.dcp_hmm_read_lodds(h.h, None) == DCP_EFUNCUSE


def test_engine_calls_check_their_arguments_without_a_gpu():
    from deciphon_amd import hip

    L = hip.load_library()
    assert L.dcp_hip_set_gencode(None, 1) == DCP_EFUNCUSE
    assert L.dcp_hip_set_gencode(None, 13) == DCP_EFUNCUSE  # NULL comes first
    assert L.dcp_hip_profile_gencode(None, 0) == 0


def test_scan_set_gencode_on_a_scan_not_set_up(capfd):
    from deciphon_amd import scan

    L = scan._lib()
    assert L.dcp_scan_set_gencode(None, 1) == DCP_EFUNCUSE
    s = L.dcp_scan_new()
    assert s
    try:
        assert L.dcp_scan_set_gencode(s, 1) == DCP_EFUNCUSE
        assert L.dcp_scan_set_gencode(s, 13) == DCP_EFUNCUSE  # not set up comes before the table
    finally:
        L.dcp_scan_del(s)
    capfd.readouterr()
