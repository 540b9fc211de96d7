"""GPU: resident profiles under another translation table, without their files (dcp_hip_set_gencode,
dcp_scan_set_gencode).

The yardstick is a fresh load: after set_gencode(t) the pool must be, word for word, the pool dcp_hip_load_hmm of the
same files and ranges leaves at (t, each profile's own error rate) -- rows, +inf padding, headers, cost-order copies,
transitions -- for every table held, every profile class and tile boundary, every DECIPHON_HIP_COST_ORDER setting and
however the profiles were loaded; a refused call must leave every word; the kernels must score and walk the rewritten
tables to the same bits; and a scan must write the products.tsv of a fresh scan under that table.  No tolerance
anywhere: the recomputation is the load's own function on the load's own inputs."""
import math
import os
import re

import numpy as np
import pytest

import translation_tables as tt
from dcp_testlib import bits
from hmm_testlib import HMM, from_hmm, pool_words, press, same_pools, synthetic_hmm, without_stops
from test_gpu_set_epsilon import LONG, SMALL, dist_bytes_of, minifam_engine, set_order
from test_gpu_translation_tables import planted_profiles, planted_reads

pytestmark = pytest.mark.gpu

DCP_EFUNCUSE, DCP_EGENCODEID = 8, 50
OTHERS = tuple(t for t in tt.IDS if t != 1)


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    """The small-classes .hmm, and the pool of a fresh load of it per (table, error rate, cost-order setting), made
    when first asked for and never changed."""
    d = tmp_path_factory.mktemp("set_gencode_small")
    hmm = synthetic_hmm(str(d / "small.hmm"), SMALL, 21)
    pools = {}

    def fresh(gc, epsilon, order=None):
        assert os.environ.get("DECIPHON_HIP_COST_ORDER") == order
        if (gc, epsilon, order) not in pools:
            pools[gc, epsilon, order] = from_hmm(hmm, gc, epsilon)
        return pools[gc, epsilon, order]

    return hmm, fresh


def refused(call, code, *args):
    import deciphon_amd

    with pytest.raises(deciphon_amd.HipError) as e:
        call(*args)
    assert e.value.code == code
    return str(e.value)


def changed(a, b):
    return any(not np.array_equal(x[2], y[2]) for x, y in zip(a, b))


# ---- the pool, word for word --------------------------------------------------------------------------------

CASES = [(None, t) for t in OTHERS] + [("0", 4), ("poison", 6)]


@pytest.mark.parametrize("order,t", CASES, ids=[f"{o or 'copies'}-1-to-{t}" for o, t in CASES])
def test_small_classes_every_boundary(small, monkeypatch, order, t):
    import deciphon_amd

    hmm, fresh = small
    set_order(monkeypatch, order)
    n = len(SMALL)
    with deciphon_amd.Engine(0) as eng:
        eng.load_hmm(hmm, 1, 0.01)
        before = pool_words(eng)
        shape = (eng.num_profiles, eng.pool_bytes, eng.dist_bytes)
        assert shape[2] == dist_bytes_of(SMALL, 1)
        assert [eng.profile_gencode(i) for i in range(n)] == [1] * n
        eng.set_gencode(t)
        after = pool_words(eng)
        assert (eng.num_profiles, eng.pool_bytes, eng.dist_bytes) == shape
        assert [eng.profile_gencode(i) for i in range(n)] == [t] * n
        assert all(eng.profile_epsilon(i) == np.float32(0.01) for i in range(n))
        assert eng.profile_gencode(n) == 0 and eng.profile_gencode(-1) == 0
        eng.set_gencode(t)  # the table that is there already: still written, still the same words
        again = pool_words(eng)
        eng.set_gencode(1)
        back = pool_words(eng)
        assert [eng.profile_gencode(i) for i in range(n)] == [1] * n
        assert (eng.num_profiles, eng.pool_bytes, eng.dist_bytes) == shape
    same_pools(before, fresh(1, 0.01, order))
    assert [(K, acc) for K, acc, _ in after] == [(K, acc) for K, acc, _ in before]
    same_pools(after, fresh(t, 0.01, order))
    same_pools(again, after)
    same_pools(back, before)
    # the comparison would pass on untouched tables if the two tables gave the same words: only 11 does, whose code is
    # table 1's (they differ in their start codons)
    assert changed(before, after) == (t != 11)
    floats = {K: len(w) for K, _, w in after}
    if order == "0":
        assert floats[300] == floats[321] and floats[640] == floats[641]
    else:
        assert floats[300] > floats[321] and floats[640] > floats[641]


def test_long_classes_through_many_chunks(tmp_path, monkeypatch):
    """Profiles beyond one wavefront's strip, and the recomputed entries go up in chunks of 1 MiB, 1985 nodes: eleven of
    them, through both pinned buffers."""
    import deciphon_amd

    set_order(monkeypatch, None)
    Ks = (LONG[2], LONG[4])
    assert Ks == (4097, 16383)
    hmm = synthetic_hmm(str(tmp_path / "long.hmm"), Ks, 22)
    want = from_hmm(hmm, 4, 0.01)
    monkeypatch.setenv("DECIPHON_HIP_STAGE_MB", "1")
    with deciphon_amd.Engine(0) as eng:
        eng.load_hmm(hmm, 1, 0.01)
        before = pool_words(eng)
        eng.set_gencode(4)
        got = pool_words(eng)
        assert eng.dist_bytes == dist_bytes_of(Ks, 1)
    assert [K for K, _, _ in got] == list(Ks)
    same_pools(got, want)
    assert changed(before, got)


# ---- engines whose profiles are under several tables and at several rates -----------------------------------

def test_two_loads_under_two_tables_at_two_rates(small, tmp_path, monkeypatch):
    import deciphon_amd

    hmm, fresh = small
    set_order(monkeypatch, None)
    Ks2 = (5, 70, 300, 1025)
    second = synthetic_hmm(str(tmp_path / "second.hmm"), Ks2, 28)
    first, count = 9, 8
    rates = [np.float32(0.01)] * count + [np.float32(0.1)] * len(Ks2)
    with deciphon_amd.Engine(0) as eng:
        eng.load_hmm(hmm, 1, 0.01, first=first, count=count)
        eng.load_hmm(second, 11, 0.1)
        n = eng.num_profiles
        assert n == count + len(Ks2)
        assert [eng.profile_gencode(i) for i in range(n)] == [1] * count + [11] * len(Ks2)
        sizes = (eng.pool_bytes, eng.dist_bytes)
        assert sizes[1] == dist_bytes_of(SMALL[first : first + count] + Ks2, 2)
        eng.set_gencode(6)
        assert [eng.profile_gencode(i) for i in range(n)] == [6] * n
        assert [eng.profile_epsilon(i) for i in range(n)] == rates
        assert (eng.pool_bytes, eng.dist_bytes) == sizes
        got = pool_words(eng)
        eng.clear_profiles()
        assert eng.dist_bytes == 0 and eng.profile_gencode(0) == 0
        eng.set_gencode(4)  # nothing kept of what was cleared
        assert eng.num_profiles == 0
    same_pools(got[:count], fresh(6, 0.01)[first : first + count])
    same_pools(got[count:], from_hmm(second, 6, 0.1))


@pytest.mark.parametrize("table_first", [True, False], ids=["gencode-then-epsilon", "epsilon-then-gencode"])
def test_with_set_epsilon_in_either_order(small, monkeypatch, table_first):
    import deciphon_amd

    hmm, fresh = small
    set_order(monkeypatch, None)
    with deciphon_amd.Engine(0) as eng:
        eng.load_hmm(hmm, 1, 0.01)
        if table_first:
            eng.set_gencode(4)
            eng.set_epsilon(0.1)
        else:
            eng.set_epsilon(0.1)
            eng.set_gencode(4)
        assert (eng.profile_gencode(0), eng.profile_epsilon(0)) == (4, np.float32(0.1))
        got = pool_words(eng)
    same_pools(got, fresh(4, 0.1))


ROW_HDR = 4  # floats in front of every emission row: null, background, 0, 0 (csrc/dcp_types.h DCP_ROW_HDR)


def canonical_rows(K, w):
    """The emission rows [1364][4 + Kp] of a profile's pool words: Kp from their number (rows, 8 transitions of Kp,
    rounded up to 32 floats; a profile without a cost-order copy)."""
    for Kp in range(64, 16384 + 1, 64):
        if Kp >= K and (1364 * (ROW_HDR + Kp) + 8 * Kp + 31) // 32 * 32 == len(w):
            return w[: 1364 * (ROW_HDR + Kp)].view(np.float32).reshape(1364, ROW_HDR + Kp)
    raise AssertionError((K, len(w)))


def test_at_epsilon_0_a_freed_stop_turns_finite(small, monkeypatch):
    """At epsilon = 0 a 3-mer costs what its codon costs: TAA is a stop under table 1, +inf in every row, and Q under
    table 6.  The pool after set_gencode(6) says so, and is the fresh load's at (6, 0)."""
    import deciphon_amd

    hmm, fresh = small
    set_order(monkeypatch, None)
    with deciphon_amd.Engine(0) as eng:
        eng.load_hmm(hmm, 1, 0.0)
        before = pool_words(eng)
        eng.set_gencode(6)
        after = pool_words(eng)
        assert eng.profile_epsilon(0) == 0.0
    same_pools(before, fresh(1, 0.0))
    same_pools(after, fresh(6, 0.0))
    taa, tga = 20 + tt.code("TAA"), 20 + tt.code("TGA")
    for (K, _, a), (_, _, b) in zip(before, after):
        if K > 64:
            continue  # (the profiles of up to 64 positions are enough, and they have no cost-order copy)
        ra, rb = canonical_rows(K, a), canonical_rows(K, b)
        assert np.isposinf(ra[taa, :2]).all() and np.isposinf(ra[taa, ROW_HDR : ROW_HDR + K]).all(), K
        assert np.isfinite(rb[taa, :2]).all() and np.isfinite(rb[taa, ROW_HDR : ROW_HDR + K]).all(), K
        assert np.isposinf(rb[tga, :2]).all() and np.isposinf(rb[tga, ROW_HDR : ROW_HDR + K]).all(), K  # still a stop under 6


# ---- refusals leave every word ------------------------------------------------------------------------------

@pytest.mark.parametrize("gc", [0, 7, 13, 34])
def test_a_table_not_held(small, monkeypatch, gc):
    import deciphon_amd

    hmm, _ = small
    set_order(monkeypatch, None)
    with deciphon_amd.Engine(0) as eng:
        eng.load_hmm(hmm, 1, 0.01, first=12, count=4)
        before = pool_words(eng)
        refused(eng.set_gencode, DCP_EGENCODEID, gc)
        same_pools(before, pool_words(eng))
        assert [eng.profile_gencode(i) for i in range(4)] == [1] * 4
        eng.set_epsilon(0.01)  # and the kept distributions are whole: the same words from them
        same_pools(before, pool_words(eng))


def _add_one(eng):
    rng = np.random.default_rng(31)
    K = 5
    eng.add_profile(K, rng.uniform(0.1, 3.0, (8, K)), rng.uniform(0.1, 9.0, (1364, K)), rng.uniform(0.1, 9.0, 1364),
                    rng.uniform(0.1, 9.0, 1364))


@pytest.mark.parametrize("other", ["load_dcp", "add_profile"])
def test_a_profile_without_distributions(small, tmp_path, monkeypatch, other):
    import deciphon_amd

    hmm, _ = small
    set_order(monkeypatch, None)
    with deciphon_amd.Engine(0) as eng:
        eng.load_hmm(hmm, 1, 0.01, first=12, count=3)
        if other == "load_dcp":
            eng.load_dcp(press(HMM, str(tmp_path / "minifam.dcp")), count=1)
        else:
            _add_one(eng)
        eng.load_hmm(hmm, 1, 0.01, first=2, count=2)
        assert [eng.profile_gencode(i) for i in range(6)] == [1, 1, 1, 0, 1, 1]
        before = pool_words(eng)
        assert "profile 3 " in refused(eng.set_gencode, DCP_EFUNCUSE, 4)
        refused(eng.set_gencode, DCP_EGENCODEID, 13)  # the table is looked at first
        same_pools(before, pool_words(eng))
        assert [eng.profile_gencode(i) for i in range(6)] == [1, 1, 1, 0, 1, 1]


def test_a_cost_batch_outstanding(monkeypatch):
    import deciphon_amd

    set_order(monkeypatch, None)
    with deciphon_amd.Engine(0) as eng:
        wins = minifam_engine(eng)
        idx0, lrt0 = eng.cost_hits(wins)
        assert len(idx0) >= 3
        before = pool_words(eng)
        eng.cost_hits_begin(wins)
        assert "outstanding" in refused(eng.set_gencode, DCP_EFUNCUSE, 4)
        assert "outstanding" in refused(eng.set_gencode, DCP_EFUNCUSE, 13)  # outstanding batches come before the table
        same_pools(before, pool_words(eng))
        idx, lrt = eng.cost_hits_end()
        assert np.array_equal(idx, idx0) and np.array_equal(lrt.view(np.uint32), lrt0.view(np.uint32))
        assert eng.profile_gencode(0) == 1
        eng.set_gencode(4)  # and once they are ended it goes through
        assert eng.profile_gencode(0) == 4


def test_it_is_a_change_of_the_inputs(monkeypatch):
    import deciphon_amd

    set_order(monkeypatch, None)
    with deciphon_amd.Engine(0) as eng:
        wins = minifam_engine(eng)
        eng.stage(wins)
        eng.run_staged(1)
        nul0, alt0 = eng.fetch_staged()
        eng.path(wins[:3], trellis=False)
        eng.path_trellis(0)
        eng.set_gencode(4)
        refused(eng.run_staged, DCP_EFUNCUSE, 1)
        refused(eng.fetch_staged, DCP_EFUNCUSE)
        refused(eng.path_trellis, DCP_EFUNCUSE, 1)
        eng.stage(wins)
        eng.run_staged(1)
        nul1, alt1 = eng.fetch_staged()
        assert not np.array_equal(alt0.view(np.uint32), alt1.view(np.uint32))
        eng.set_gencode(4)  # the table that is there already: a change all the same
        refused(eng.run_staged, DCP_EFUNCUSE, 1)


def test_engine_without_profiles():
    import deciphon_amd

    with deciphon_amd.Engine(0) as eng:
        eng.set_gencode(4)
        assert eng.num_profiles == 0 and eng.dist_bytes == 0 and eng.profile_gencode(0) == 0
        refused(eng.set_gencode, DCP_EGENCODEID, 13)


# ---- the kernels read it --------------------------------------------------------------------------------------

def test_kernels_score_an_in_frame_taa_after_the_change(tmp_path, monkeypatch):
    """One profile per kernel family -- K = 3 (a pack), 173 (one wavefront), 300 ((5,1), with its cost-order copy) and
    768 (several wavefronts) -- at epsilon = 0 on a window with TAA in frame and no stop of table 6: +inf under table 1,
    and after set_gencode(6) the bits, and the path steps, of an engine loaded under 6."""
    import deciphon_amd

    set_order(monkeypatch, None)
    Ks = (3, 173, 300, 768)
    hmm = synthetic_hmm(str(tmp_path / "four.hmm"), Ks, 24)
    L = 300
    x = np.random.default_rng(6).integers(0, 4, size=L).astype(np.uint8)
    for at in (30, 150, 291):
        x[at : at + 3] = tt.indices("TAA")
    x = without_stops(x, tt.stops(6))
    text = "".join("ACGT"[v] for v in x)
    assert "TGA" not in text and all(text[at : at + 3] == "TAA" for at in (30, 150, 291))
    wins = [(i, 0, 0, L) for i in range(len(Ks))]

    def ready(eng, gc):
        eng.load_hmm(hmm, gc, 0.0)
        eng.commit()
        eng.set_sequences([x])
        eng.set_mode(True, False)

    def score(eng):
        nul, alt = eng.cost(wins)
        return nul, alt, eng.path(wins, trellis=False)

    with deciphon_amd.Engine(0) as eng:
        ready(eng, 1)
        nul1, alt1 = eng.cost(wins)
        eng.set_gencode(6)
        got = score(eng)
    with deciphon_amd.Engine(0) as eng:
        ready(eng, 6)
        want = score(eng)
    assert np.isposinf(nul1).all() and np.isposinf(alt1).all()
    assert np.isfinite(want[0]).all() and np.isfinite(want[1]).all()
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
    for K, a, b in zip(Ks, got[2], want[2]):
        assert bits(a["score"]) == bits(b["score"]), K
        assert len(a["state_ids"]) > 10, K
        assert np.array_equal(a["state_ids"], b["state_ids"]) and np.array_equal(a["seqsizes"], b["seqsizes"]), K


# ---- the scan -------------------------------------------------------------------------------------------------

def planted_scan(tmp_path, gc):
    from deciphon_amd import synth
    from deciphon_amd.scan import Batch, Sequence

    profiles = planted_profiles(gc)
    hmm = str(tmp_path / "planted.hmm")
    synth.write_hmm(hmm, profiles)
    batch = Batch()
    for sid, text in planted_reads(gc, profiles):
        batch.add(Sequence(sid, f"r{sid}", text))
    return hmm, batch


# 4: TGA spells W, a stop under table 1 (whose scan of these reads finds nothing); 12: CTG spells S, and L under table 1
# (both scans have rows, and the amino column tells them apart)
@pytest.mark.parametrize("gc", [4, 12])
def test_scan_set_gencode(tmp_path, monkeypatch, gc):
    from deciphon_amd.scan import DeciphonError, Scan

    set_order(monkeypatch, None)
    hmm, batch = planted_scan(tmp_path, gc)

    def run(scan, name):
        scan.run(str(tmp_path / name), batch)
        return open(tmp_path / name / "products.tsv", "rb").read()

    with Scan.from_hmm(hmm, gc, 0.01) as scan:
        fresh_t = run(scan, "fresh_t")
    assert len(fresh_t.splitlines()) >= 3
    with Scan.from_hmm(hmm, 1, 0.01) as scan:
        fresh_1 = run(scan, "fresh_1")
        rows_1 = scan.products()
        assert fresh_1 != fresh_t  # or the comparison below would pass on untouched tables
        scan.set_gencode(gc)
        assert scan.products() == rows_1  # the rows of the last run stay
        assert run(scan, "switched_t") == fresh_t
        scan.set_gencode(1)
        assert run(scan, "back_1") == fresh_1
        scan.set_gencode(gc)
        with pytest.raises(DeciphonError) as e:
            scan.set_gencode(13)
        assert e.value.code == DCP_EGENCODEID
        assert run(scan, "still_t") == fresh_t
        scan.set_epsilon(0.01)  # the two changes go together
        assert run(scan, "same_rate_t") == fresh_t


def test_scan_of_a_pressed_file_is_refused(tmp_path, monkeypatch):
    from deciphon_amd.scan import DeciphonError, Scan

    set_order(monkeypatch, None)
    hmm, batch = planted_scan(tmp_path, 12)
    dcp = press(hmm, str(tmp_path / "planted.dcp"), 12, 0.01)
    with Scan(dcp, 0, 1, True, False, False) as scan:
        scan.run(str(tmp_path / "before"), batch)
        with pytest.raises(DeciphonError) as e:
            scan.set_gencode(1)
        assert e.value.code == DCP_EFUNCUSE
        with pytest.raises(DeciphonError) as e:
            scan.set_gencode(13)
        assert e.value.code == DCP_EFUNCUSE  # a pressed file comes before the table
        scan.run(str(tmp_path / "after"), batch)
    before = open(tmp_path / "before" / "products.tsv", "rb").read()
    assert len(before.splitlines()) >= 3 and before == open(tmp_path / "after" / "products.tsv", "rb").read()


# ---- the timing line ------------------------------------------------------------------------------------------

def test_timing_line(small, monkeypatch, capfd):
    import deciphon_amd

    hmm, _ = small
    set_order(monkeypatch, None)
    monkeypatch.setenv("DECIPHON_HIP_TIMING", "1")
    with deciphon_amd.Engine(0) as eng:
        eng.load_hmm(hmm, 1, 0.01)
        capfd.readouterr()
        eng.set_gencode(11)
        err = capfd.readouterr().err
    line = re.findall(r"dcp_hip_set_gencode: (\d+) profiles, (\d+) nodes, .*host recomputation ([\d.]+) s, upload ([\d.]+) s, "
                      r"kernels ([\d.]+) s", err)
    assert len(line) == 1, err
    assert (int(line[0][0]), int(line[0][1])) == (len(SMALL), sum(SMALL))
    assert all(math.isfinite(float(v)) and float(v) >= 0 for v in line[0][2:])
