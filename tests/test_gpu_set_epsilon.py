"""GPU: resident profiles at a new error rate, in place (dcp_hip_set_epsilon, dcp_scan_set_epsilon;
csrc/press_reemit.hip).

The yardstick is a fresh load: after set_epsilon(e) the pool must be, word for word, the pool dcp_hip_load_hmm of the
same files, ranges and translation table leaves at e -- rows, +inf padding, headers, cost-order copies, transitions --
for every profile class and tile boundary, every DECIPHON_HIP_COST_ORDER setting and however the profiles were loaded;
a refused call must leave every word; the kernels must score and walk the rewritten tables to the same bits; and a
scan must write the products.tsv of a fresh scan at that rate."""
import math
import os
import re

import numpy as np
import pytest

from dcp_testlib import GOLDEN, bits, read_fasta
from hmm_testlib import HMM, from_hmm, pool_words, press, same_pools, synthetic_hmm

pytestmark = pytest.mark.gpu

# the shapes of the load's own test (test_gpu_load_hmm.py): a single node, a tile edge at 63, 64 and 65, Kp = 128 for
# K = 61..64, both cost-order shapes at both ends and their neighbours without a copy; every profile crosses the last
# code tile, which holds 20 codes
SMALL = (1, 2, 3, 12, 13, 60, 61, 64, 65, 124, 125, 256, 257, 300, 320, 321, 448, 449, 512, 513, 640, 641, 768, 769, 1024)
LONG = (2048, 4096, 4097, 8193, 16383)
DCP_EFUNCUSE, DCP_ELARGECORESIZE = 8, 63
ENTRY = 528  # bytes of one kept entry: nucltp[4], codonm[125], 3 floats of padding


def dist_bytes_of(core_sizes, loads):
    """What dcp_hip_dist_bytes must say: one entry per node of every profile, and per dcp_hip_load_hmm that added
    profiles two more, its null model and its background."""
    return ENTRY * (sum(core_sizes) + 2 * loads)


def set_order(monkeypatch, order):
    if order is None:
        monkeypatch.delenv("DECIPHON_HIP_COST_ORDER", raising=False)
    else:
        monkeypatch.setenv("DECIPHON_HIP_COST_ORDER", order)


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    """The small-classes .hmm, and the pool of a fresh load of it per (cost-order setting, error rate), made when first
    asked for and never changed."""
    d = tmp_path_factory.mktemp("set_epsilon_small")
    hmm = synthetic_hmm(str(d / "small.hmm"), SMALL, 21)
    pools = {}

    def fresh(epsilon, order=None):
        assert os.environ.get("DECIPHON_HIP_COST_ORDER") == order
        if (order, epsilon) not in pools:
            pools[(order, epsilon)] = from_hmm(hmm, 1, epsilon)
        return pools[(order, epsilon)]

    return hmm, fresh


def refused(call, *args):
    import deciphon_amd

    with pytest.raises(deciphon_amd.HipError) as e:
        call(*args)
    assert e.value.code == DCP_EFUNCUSE
    return str(e.value)


# ---- (a), (b): the pool, word for word ------------------------------------------------------------------

PAIRS = [(0.01, 0.1), (0.1, 0.01), (0.01, 0.0), (0.0, 0.01), (0.01, 1e-30), (0.01, 1.0)]
CASES = [(None, p) for p in PAIRS] + [("0", p) for p in PAIRS] + [("poison", PAIRS[0])]


@pytest.mark.parametrize("order,pair", CASES, ids=[f"{o or 'copies'}-{a}-{b}" for o, (a, b) in CASES])
def test_small_classes_every_boundary(small, monkeypatch, order, pair):
    import deciphon_amd

    hmm, fresh = small
    set_order(monkeypatch, order)
    e0, e1 = pair
    with deciphon_amd.Engine(0) as eng:
        eng.load_hmm(hmm, 1, e0)
        before = pool_words(eng)
        shape = (eng.num_profiles, eng.pool_bytes)
        assert eng.dist_bytes == dist_bytes_of(SMALL, 1)
        assert all(eng.profile_epsilon(i) == np.float32(e0) for i in range(len(SMALL)))
        eng.set_epsilon(e1)
        after = pool_words(eng)
        assert (eng.num_profiles, eng.pool_bytes) == shape
        assert eng.dist_bytes == dist_bytes_of(SMALL, 1)
        assert all(eng.profile_epsilon(i) == np.float32(e1) for i in range(len(SMALL)))
        assert math.isnan(eng.profile_epsilon(len(SMALL))) and math.isnan(eng.profile_epsilon(-1))
    same_pools(before, fresh(e0, order))
    assert [(K, acc) for K, acc, _ in after] == [(K, acc) for K, acc, _ in before]  # core sizes and accessions
    same_pools(after, fresh(e1, order))
    # the comparison would pass on untouched tables if the two rates gave the same words
    assert any(not np.array_equal(a[2], b[2]) for a, b in zip(before, after))
    floats = {K: len(w) for K, _, w in after}
    if order == "0":
        assert floats[300] == floats[321] and floats[640] == floats[641]
    else:
        assert floats[300] > floats[321] and floats[640] > floats[641]


def test_round_trip(small, monkeypatch):
    import deciphon_amd

    hmm, fresh = small
    set_order(monkeypatch, None)
    with deciphon_amd.Engine(0) as eng:
        eng.load_hmm(hmm, 1, 0.01)
        first = pool_words(eng)
        eng.set_epsilon(0.1)
        eng.set_epsilon(0.1)  # what is there already: still written, still the same
        same_pools(pool_words(eng), fresh(0.1))
        eng.set_epsilon(0.01)
        same_pools(pool_words(eng), first)
    same_pools(first, fresh(0.01))


def test_engine_without_profiles(monkeypatch):
    import deciphon_amd

    with deciphon_amd.Engine(0) as eng:
        eng.set_epsilon(0.1)
        assert eng.num_profiles == 0 and eng.dist_bytes == 0 and math.isnan(eng.profile_epsilon(0))


# ---- (c): profiles beyond one wavefront's strip ---------------------------------------------------------

def test_long_classes(tmp_path, monkeypatch):
    import deciphon_amd

    set_order(monkeypatch, None)
    hmm = synthetic_hmm(str(tmp_path / "long.hmm"), LONG, 22)
    with deciphon_amd.Engine(0) as eng:
        eng.load_hmm(hmm, 1, 0.01)
        eng.set_epsilon(0.1)
        got = pool_words(eng)
        assert eng.dist_bytes == dist_bytes_of(LONG, 1)
    assert [K for K, _, _ in got] == list(LONG)
    same_pools(got, from_hmm(hmm, 1, 0.1))


# ---- (d): how it was loaded must not matter -------------------------------------------------------------

def test_batches_of_300_nodes(small, monkeypatch):
    import deciphon_amd

    hmm, fresh = small
    set_order(monkeypatch, None)
    want = fresh(0.1)
    monkeypatch.setenv("DECIPHON_HIP_PRESS_BATCH_NODES", "300")
    with deciphon_amd.Engine(0) as eng:
        eng.load_hmm(hmm, 1, 0.01)
        eng.set_epsilon(0.1)
        same_pools(pool_words(eng), want)


def test_two_loads_at_two_rates(small, tmp_path, monkeypatch):
    import deciphon_amd

    hmm, fresh = small
    set_order(monkeypatch, None)
    long2 = synthetic_hmm(str(tmp_path / "long2.hmm"), LONG[:2], 27)
    first, count = 9, 8
    with deciphon_amd.Engine(0) as eng:
        eng.load_hmm(hmm, 1, 0.01, first=first, count=count)
        eng.load_hmm(long2, 1, 0.05)
        assert eng.num_profiles == count + 2
        assert [eng.profile_epsilon(i) for i in range(count + 2)] == [np.float32(0.01)] * count + [np.float32(0.05)] * 2
        assert eng.dist_bytes == dist_bytes_of(SMALL[first : first + count] + LONG[:2], 2)
        eng.set_epsilon(0.1)
        assert [eng.profile_epsilon(i) for i in range(count + 2)] == [np.float32(0.1)] * (count + 2)
        got = pool_words(eng)
        eng.clear_profiles()
        assert eng.dist_bytes == 0
    same_pools(got[:count], fresh(0.1)[first : first + count])
    same_pools(got[count:], from_hmm(long2, 1, 0.1))


def _unannounced(text):
    """The file with every `LENG  K` written `LENG<TAB>K`: the profile parser splits on any whitespace and reads it
    alike, but the pass that sizes the pool and the kept distributions looks for "LENG " and finds nothing to size
    them by."""
    out, n = re.subn(r"^LENG +(\d+)$", "LENG\t\\1", text, flags=re.M)
    assert n == len(SMALL)
    return out


def test_distributions_grow_during_the_load(small, tmp_path, monkeypatch, capfd):
    """No announced lengths, batches of 300 nodes: the buffer of kept distributions is reallocated batch by batch, as
    the pool is, while the other slot's batch may be in flight."""
    import deciphon_amd

    hmm, fresh = small
    set_order(monkeypatch, None)
    want = fresh(0.1)
    tabbed = tmp_path / "tabbed.hmm"
    tabbed.write_text(_unannounced(open(hmm).read()))
    monkeypatch.setenv("DECIPHON_HIP_PRESS_BATCH_NODES", "300")
    monkeypatch.setenv("DECIPHON_HIP_TIMING", "1")
    with deciphon_amd.Engine(0) as eng:
        capfd.readouterr()
        eng.load_hmm(str(tabbed), 1, 0.01)
        err = capfd.readouterr().err
        assert [int(n) for n in re.findall(r"pool grown (\d+) times", err)][0] >= 2
        assert [int(n) for n in re.findall(r"kept (\d+) bytes of distributions", err)] == [dist_bytes_of(SMALL, 1)]
        assert eng.dist_bytes == dist_bytes_of(SMALL, 1)
        eng.set_epsilon(0.1)
        line = re.findall(r"dcp_hip_set_epsilon: (\d+) profiles, (\d+) nodes, (\d+) bytes written", capfd.readouterr().err)
        assert [(int(a), int(b)) for a, b, _ in line] == [(len(SMALL), sum(SMALL))]
        same_pools(pool_words(eng), want)


# ---- (e): refusals leave every word ---------------------------------------------------------------------

@pytest.mark.parametrize("epsilon", [-0.1, 1.5, float("nan")])
def test_epsilon_out_of_range(small, monkeypatch, epsilon):
    import deciphon_amd

    hmm, _ = small
    set_order(monkeypatch, None)
    with deciphon_amd.Engine(0) as eng:
        eng.load_hmm(hmm, 1, 0.01, first=12, count=4)
        before = pool_words(eng)
        refused(eng.set_epsilon, epsilon)
        same_pools(before, pool_words(eng))
        assert [eng.profile_epsilon(i) for i in range(4)] == [np.float32(0.01)] * 4


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
        assert math.isnan(eng.profile_epsilon(3)) and eng.profile_epsilon(4) == np.float32(0.01)
        assert eng.dist_bytes == dist_bytes_of(SMALL[12:15] + SMALL[2:4], 2)
        before = pool_words(eng)
        assert "profile 3 " in refused(eng.set_epsilon, 0.1)
        same_pools(before, pool_words(eng))


def minifam_engine(eng):
    """minifam at 0.01 and its consensus reads, ready to score; -> windows, the first three of them hits."""
    import deciphon_amd

    reads = [deciphon_amd.encode(s) for _, s in read_fasta(os.path.join(GOLDEN, "consensus.fna"))]
    eng.load_hmm(HMM, 1, 0.01)
    eng.commit()
    eng.set_sequences(reads)
    eng.set_mode(True, False)
    return [(i, i, 0, len(reads[i])) for i in range(3)] + [(i, (i + 1) % 3, 0, 200) for i in range(3)]


def test_a_cost_batch_outstanding(monkeypatch):
    import deciphon_amd

    set_order(monkeypatch, None)
    with deciphon_amd.Engine(0) as eng:
        wins = minifam_engine(eng)
        idx0, lrt0 = eng.cost_hits(wins)
        assert len(idx0) >= 3
        before = pool_words(eng)
        eng.cost_hits_begin(wins)
        assert "outstanding" in refused(eng.set_epsilon, 0.1)
        same_pools(before, pool_words(eng))
        idx, lrt = eng.cost_hits_end()
        assert np.array_equal(idx, idx0) and np.array_equal(lrt.view(np.uint32), lrt0.view(np.uint32))
        assert eng.profile_epsilon(0) == np.float32(0.01)
        eng.set_epsilon(0.1)  # and once they are ended it goes through
        assert eng.profile_epsilon(0) == np.float32(0.1)


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
        eng.set_epsilon(0.1)
        refused(eng.run_staged, 1)
        refused(eng.fetch_staged)
        refused(eng.path_trellis, 1)
        eng.stage(wins)
        eng.run_staged(1)
        nul1, alt1 = eng.fetch_staged()
        assert not np.array_equal(alt0.view(np.uint32), alt1.view(np.uint32))
        eng.path(wins[:3], trellis=False)
        eng.path_trellis(1)
        eng.set_epsilon(0.1)  # the rate that is there already: a change all the same
        refused(eng.run_staged, 1)
        refused(eng.path_trellis, 2)


def test_after_a_load_that_failed(small, tmp_path, monkeypatch):
    """A failed load has written its distributions behind the kept ones, as its tables behind the pool: none of it
    counts, and the kept ones are whole."""
    import deciphon_amd

    hmm, fresh = small
    set_order(monkeypatch, None)
    big = synthetic_hmm(str(tmp_path / "big.hmm"), (5, 16384, 7), 23)
    with deciphon_amd.Engine(0) as eng:
        eng.load_hmm(hmm, 1, 0.01, count=4)
        with pytest.raises(deciphon_amd.HipError) as e:
            eng.load_hmm(big, 1, 0.05)
        assert e.value.code == DCP_ELARGECORESIZE
        assert eng.num_profiles == 4 and eng.dist_bytes == dist_bytes_of(SMALL[:4], 1)
        eng.set_epsilon(0.1)
        same_pools(pool_words(eng), fresh(0.1)[:4])


# ---- (f): the kernels read it ---------------------------------------------------------------------------

def test_kernels_read_what_was_written(tmp_path, monkeypatch):
    """One profile per kernel family -- K = 3 (a pack), 173, 300 and 640 (the two cost-order shapes, with their
    copies), 768, 1024 -- scored and walked after set_epsilon as by an engine loaded at that rate."""
    import deciphon_amd
    from deciphon_amd import synth
    from deciphon_amd.host import HmmFile

    set_order(monkeypatch, None)
    Ks = (3, 173, 300, 640, 768, 1024)
    hmm = synthetic_hmm(str(tmp_path / "six.hmm"), Ks, 24)
    with HmmFile(hmm) as h:
        consensus = [p["consensus"] for p in h]
    rng = np.random.default_rng(25)
    read = rng.integers(0, 4, size=4000).astype(np.uint8)
    planted, at = [], 100
    for cons in consensus:  # a mutated copy of (up to 120 residues of) each profile's consensus
        dom = synth.mutate(synth.back_translate(cons[:120]), rng, 0.05, 0.01, 0.01)
        read[at : at + len(dom)] = dom
        planted.append((max(at - 60, 0), min(at + len(dom) + 60, len(read))))
        at += len(dom) + 150
    assert at < len(read)
    wins, hit_wins = [], []
    for p in range(len(Ks)):
        hit_wins.append(len(wins))
        wins.append((p, 0, *planted[p]))
        for n in (30, 31, 32, 299, 300, 301, 600):  # multiples of 3 and not
            a = int(rng.integers(0, 3300))
            wins.append((p, 0, a, a + n))

    def score(eng):
        nul, alt = eng.cost(wins)
        return nul, alt, eng.path([wins[i] for i in hit_wins], trellis=False)

    def ready(eng, epsilon):
        eng.load_hmm(hmm, 1, epsilon)
        eng.commit()
        eng.set_sequences([read])
        eng.set_mode(True, False)

    got, want = {}, {}
    with deciphon_amd.Engine(0) as eng:
        ready(eng, 0.01)
        at_001 = score(eng)
        for epsilon in (0.1, 0.0):
            eng.set_epsilon(epsilon)
            got[epsilon] = score(eng)
    for epsilon in (0.1, 0.0):
        with deciphon_amd.Engine(0) as eng:
            ready(eng, epsilon)
            want[epsilon] = score(eng)
    assert not np.array_equal(at_001[1].view(np.uint32), want[0.1][1].view(np.uint32))
    assert np.isfinite(want[0.1][1][hit_wins]).all()
    for epsilon in (0.1, 0.0):
        (nul_a, alt_a, paths_a), (nul_b, alt_b, paths_b) = got[epsilon], want[epsilon]
        assert np.array_equal(nul_a.view(np.uint32), nul_b.view(np.uint32)), epsilon
        assert np.array_equal(alt_a.view(np.uint32), alt_b.view(np.uint32)), epsilon
        for K, a, b in zip(Ks, paths_a, paths_b):
            assert bits(a["score"]) == bits(b["score"]), (epsilon, K)
            assert np.array_equal(a["state_ids"], b["state_ids"]) and np.array_equal(a["seqsizes"], b["seqsizes"]), (epsilon, K)
            if epsilon == 0.1:
                assert len(a["state_ids"]) > 10, K


# ---- (g): the scan --------------------------------------------------------------------------------------

def indel_batch():
    """The consensus reads, and copies of the first two with one base deleted and one inserted inside the domain."""
    from deciphon_amd.scan import Batch, Sequence

    reads = [s for _, s in read_fasta(os.path.join(GOLDEN, "consensus.fna"))]
    for s in reads[:2]:
        assert len(s) > 400
        reads.append(s[:100] + s[101:300] + "G" + s[300:])
    batch = Batch()
    for i, s in enumerate(reads):
        batch.add(Sequence(i, f"seq{i}", s))
    return batch


def match_step_lengths(tsv):
    lengths = set()
    for line in open(tsv).read().splitlines()[1:]:
        for step in line.split("\t")[11].split(";"):
            nt, state = step.split(",")[:2]
            if state.startswith("M"):
                lengths.add(len(nt))
    return lengths


def test_scan_set_epsilon(tmp_path, monkeypatch):
    from deciphon_amd.scan import DeciphonError, Scan

    set_order(monkeypatch, None)
    batch = indel_batch()

    def run(scan, name):
        scan.run(str(tmp_path / name), batch)
        return open(tmp_path / name / "products.tsv", "rb").read()

    with Scan.from_hmm(HMM, 1, 0.1) as scan:
        fresh_01 = run(scan, "fresh_0.1")
    with Scan.from_hmm(HMM, 1, 0.01) as scan:
        fresh_001 = run(scan, "fresh_0.01")
        rows_001 = scan.products()
        assert match_step_lengths(tmp_path / "fresh_0.01" / "products.tsv") - {3}
        assert fresh_001 != fresh_01  # or the comparison below would pass on untouched tables
        scan.set_epsilon(0.1)
        assert scan.products() == rows_001  # the rows of the last run stay
        assert run(scan, "switched_0.1") == fresh_01
        scan.set_epsilon(0.01)
        assert run(scan, "back_0.01") == fresh_001
        with pytest.raises(DeciphonError) as e:
            scan.set_epsilon(1.5)
        assert e.value.code == DCP_EFUNCUSE
        assert run(scan, "still_0.01") == fresh_001


def test_scan_of_a_pressed_file_is_refused(tmp_path, monkeypatch):
    from deciphon_amd.scan import DeciphonError, Scan

    set_order(monkeypatch, None)
    batch = indel_batch()
    with Scan(os.path.join(GOLDEN, "minifam.dcp"), 0, 1, True, False, False) as scan:
        scan.run(str(tmp_path / "before"), batch)
        with pytest.raises(DeciphonError) as e:
            scan.set_epsilon(0.1)
        assert e.value.code == DCP_EFUNCUSE
        scan.run(str(tmp_path / "after"), batch)
    before = open(tmp_path / "before" / "products.tsv", "rb").read()
    assert len(before.splitlines()) > 3 and before == open(tmp_path / "after" / "products.tsv", "rb").read()
