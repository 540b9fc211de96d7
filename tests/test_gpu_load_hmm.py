"""GPU: straight from a HMMER3 file into HBM (dcp_hip_load_hmm, dcp_scan_setup_hmm; csrc/press_rows.hip).

The yardstick is the route through a file: dcp_press_* to a temporary .dcp, then dcp_hip_load_dcp.  The pool a load
from the .hmm leaves must be that pool word for word -- rows, +inf padding, headers, transitions, cost-order copies --
for every profile class and boundary, every error rate, every DECIPHON_HIP_COST_ORDER setting, any batching and any
range; the kernels must score and walk it to the same bits; and a scan set up from the .hmm must write the rows of a
scan of the pressed file (and, for minifam, the reference's products.tsv)."""
import os

import numpy as np
import pytest

from dcp_testlib import GOLDEN, bits, read_fasta
from hmm_testlib import HMM, from_file, from_hmm, pool_words, press, same_pools, synthetic_hmm

pytestmark = pytest.mark.gpu

SMALL = (1, 2, 3, 12, 13, 60, 61, 64, 65, 124, 125, 256, 257, 300, 320, 321, 448, 449, 512, 513, 640, 641, 768, 769, 1024)
LONG = (2048, 4096, 4097, 8193, 16383)
DCP_EZEROMODEL, DCP_ELARGECORESIZE = 12, 63


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    """The small-classes .hmm and its pressed files, one per error rate, pressed when first asked for."""
    d = tmp_path_factory.mktemp("load_hmm_small")
    hmm = synthetic_hmm(str(d / "small.hmm"), SMALL, 21)
    pressed = {}

    def dcp(epsilon):
        if epsilon not in pressed:
            pressed[epsilon] = press(hmm, str(d / f"small_{epsilon}.dcp"), 1, epsilon)
        return pressed[epsilon]

    return hmm, dcp


# ---- the pool, byte for byte ----------------------------------------------------------------------------

@pytest.mark.parametrize("order", [None, "0", "poison"], ids=["copies", "no-copies", "poison"])
@pytest.mark.parametrize("epsilon", [0.0, 0.01, 0.1])
def test_small_classes_every_boundary(small, monkeypatch, epsilon, order):
    hmm, dcp = small
    if order is None:
        monkeypatch.delenv("DECIPHON_HIP_COST_ORDER", raising=False)
    else:
        monkeypatch.setenv("DECIPHON_HIP_COST_ORDER", order)
    a = from_file(dcp(epsilon))
    b = from_hmm(hmm, 1, epsilon)
    assert [K for K, _, _ in b] == list(SMALL)
    same_pools(a, b)
    # the sizes say where the copies are: K = 257..320 and 513..640 share their classes with 321 and 641
    floats = {K: len(w) for K, _, w in b}
    if order == "0":
        assert floats[300] == floats[321] and floats[640] == floats[641]
    else:
        assert floats[300] > floats[321] and floats[640] > floats[641]
    if epsilon == 0.0:  # +inf went through the sign flip, and no NaN came of it
        w = b[SMALL.index(13)][2].view(np.float32)
        assert np.isposinf(w).any() and not np.isnan(w).any() and not np.isneginf(w).any()


def test_long_classes(tmp_path):
    hmm = synthetic_hmm(str(tmp_path / "long.hmm"), LONG, 22)
    dcp = press(hmm, str(tmp_path / "long.dcp"))
    a = from_file(dcp)
    os.unlink(dcp)
    b = from_hmm(hmm)
    assert [K for K, _, _ in b] == list(LONG)
    same_pools(a, b)


def test_core_size_16384_is_refused(small, tmp_path):
    import deciphon_amd

    hmm, _ = small
    big = synthetic_hmm(str(tmp_path / "big.hmm"), (5, 16384, 7), 23)
    with deciphon_amd.Engine(0) as eng:
        eng.load_hmm(hmm, count=4)
        before = (eng.num_profiles, eng.pool_bytes, pool_words(eng))
        with pytest.raises(deciphon_amd.HipError) as e:
            eng.load_hmm(big)
        assert e.value.code == DCP_ELARGECORESIZE
        assert (eng.num_profiles, eng.pool_bytes) == before[:2] == (4, before[1])
        same_pools(before[2], pool_words(eng))


def test_batches_of_300_nodes(small, monkeypatch):
    hmm, _ = small
    whole = from_hmm(hmm)
    monkeypatch.setenv("DECIPHON_HIP_PRESS_BATCH_NODES", "300")
    same_pools(whole, from_hmm(hmm))


def test_ranges_and_appending(small, tmp_path):
    import deciphon_amd

    hmm, _ = small
    whole = from_hmm(hmm)
    same_pools(whole[2:5], from_hmm(hmm, first=2, count=3))
    same_pools(whole[20:], from_hmm(hmm, first=20))
    assert from_hmm(hmm, first=len(SMALL)) == []
    minifam = os.path.join(GOLDEN, "minifam.dcp")
    with deciphon_amd.Engine(0) as eng:
        eng.load_dcp(minifam)
        first3 = pool_words(eng)
        assert len(first3) == 3
        eng.load_hmm(hmm, first=10, count=6)
        assert eng.num_profiles == 9
        same_pools(first3, pool_words(eng, 0, 3))
        same_pools(whole[10:16], pool_words(eng, 3))
        # a first out of range, and a file whose third profile is broken: nothing is added, nothing moves
        state = (eng.num_profiles, eng.pool_bytes)
        with pytest.raises(deciphon_amd.HipError) as e:
            eng.load_hmm(hmm, first=len(SMALL) + 1)
        assert e.value.code == 40  # DCP_EINVALPART
        good = open(HMM).read()
        one = good[: good.index("//\n") + 3]
        bad = tmp_path / "bad.hmm"
        bad.write_text(one + one + one.replace("LENG  173", "LENG  0") + one)
        with pytest.raises(deciphon_amd.HipError) as e:
            eng.load_hmm(str(bad))
        assert e.value.code == DCP_EZEROMODEL
        assert (eng.num_profiles, eng.pool_bytes) == state
        same_pools(first3, pool_words(eng, 0, 3))
        same_pools(whole[10:16], pool_words(eng, 3))


def _unannounced(text):
    """The file with every `LENG  K` written `LENG<TAB>K`: the profile parser splits on any whitespace and reads it
    alike, but the pass that sizes the pool looks for "LENG " and finds nothing to size it by."""
    import re

    out, n = re.subn(r"^LENG +(\d+)$", "LENG\t\\1", text, flags=re.M)
    assert n == len(SMALL)
    return out


def test_pool_grows_during_a_load(small, tmp_path, monkeypatch, capfd):
    """A file that announces no lengths, in batches of 300 nodes behind three resident profiles: the pool is
    reallocated batch by batch -- a stream sync, a new allocation and a copy of what is written, while the other
    slot's batch may be in flight.  DECIPHON_HIP_TIMING's line is the witness that it was; the words and the scores
    are those of the untouched file, whose load sizes the pool once."""
    import re

    import deciphon_amd
    from deciphon_amd.host import HmmFile

    hmm, _ = small
    tabbed = tmp_path / "tabbed.hmm"
    tabbed.write_text(_unannounced(open(hmm).read()))
    with HmmFile(str(tabbed)) as h:  # the parser reads it alike
        assert [p["core_size"] for p in h] == list(SMALL)
    minifam = os.path.join(GOLDEN, "minifam.dcp")
    rng = np.random.default_rng(26)
    read = rng.integers(0, 4, size=1500).astype(np.uint8)
    wins = [(p, 0, a, a + n) for p in (3, 3 + len(SMALL) // 2, 3 + len(SMALL) - 1)
            for a, n in zip(rng.integers(0, 700, size=5).tolist(), rng.integers(30, 700, size=5).tolist())]
    monkeypatch.setenv("DECIPHON_HIP_PRESS_BATCH_NODES", "300")
    monkeypatch.setenv("DECIPHON_HIP_TIMING", "1")
    got = []
    for path in (hmm, str(tabbed)):
        with deciphon_amd.Engine(0) as eng:
            eng.load_dcp(minifam)
            resident = pool_words(eng)
            assert len(resident) == 3
            capfd.readouterr()
            eng.load_hmm(path)
            grown = [int(n) for n in re.findall(r"pool grown (\d+) times", capfd.readouterr().err)]
            words = pool_words(eng)
            same_pools(resident, words[:3])
            eng.commit()
            eng.set_sequences([read])
            eng.set_mode(True, False)
            nul, alt = eng.cost(wins)
        got.append((grown, words, nul, alt))
    (grown_a, words_a, nul_a, alt_a), (grown_b, words_b, nul_b, alt_b) = got
    assert len(grown_a) == len(grown_b) == 1
    assert grown_a[0] <= 1 and grown_b[0] >= 2, (grown_a, grown_b)
    assert [K for K, _, _ in words_b[3:]] == list(SMALL)
    same_pools(words_a, words_b)
    assert np.isfinite(alt_a).all()
    assert np.array_equal(nul_a.view(np.uint32), nul_b.view(np.uint32))
    assert np.array_equal(alt_a.view(np.uint32), alt_b.view(np.uint32))


def test_load_that_fails_after_growth_leaves_the_pool(small, tmp_path, monkeypatch, capfd):
    """The last profile says LENG<TAB>0: the load fails in its last batch, after the pool was reallocated under the
    resident profiles.  They, their number and pool_bytes are what they were, and a load after it finds them so."""
    import re

    import deciphon_amd

    hmm, _ = small
    text = _unannounced(open(hmm).read())
    at = text.rindex(f"LENG\t{SMALL[-1]}\n")
    bad = tmp_path / "bad.hmm"
    bad.write_text(text[:at] + "LENG\t0\n" + text[at + len(f"LENG\t{SMALL[-1]}\n") :])
    good = tmp_path / "tabbed.hmm"
    good.write_text(text)
    monkeypatch.setenv("DECIPHON_HIP_PRESS_BATCH_NODES", "300")
    monkeypatch.setenv("DECIPHON_HIP_TIMING", "1")
    with deciphon_amd.Engine(0) as eng:
        eng.load_dcp(os.path.join(GOLDEN, "minifam.dcp"))
        before = (eng.num_profiles, eng.pool_bytes, pool_words(eng))
        with pytest.raises(deciphon_amd.HipError) as e:
            eng.load_hmm(str(bad))
        assert e.value.code == DCP_EZEROMODEL
        assert (eng.num_profiles, eng.pool_bytes) == before[:2]
        same_pools(before[2], pool_words(eng))
        # the pool did grow under them: the same file without its last profile's fault fits without a reallocation
        capfd.readouterr()
        eng.load_hmm(str(good), count=len(SMALL) - 1)
        assert [int(n) for n in re.findall(r"pool grown (\d+) times", capfd.readouterr().err)] == [0]
        same_pools(before[2], pool_words(eng, 0, 3))
        assert eng.num_profiles == 3 + len(SMALL) - 1


def test_kernels_read_what_was_written(tmp_path):
    """K = 3 (a pack), 173 ((3,1)), 300 and 600 (the two cost-order shapes), 700 (two waves): the descriptors
    (cost_shape, the offsets) are not in the pool words -- the scores and a path are what checks them."""
    import deciphon_amd
    from deciphon_amd import synth
    from deciphon_amd.host import Database

    Ks = (3, 173, 300, 600, 700)
    hmm = synthetic_hmm(str(tmp_path / "five.hmm"), Ks, 24)
    dcp = press(hmm, str(tmp_path / "five.dcp"))
    db = Database(dcp)
    consensus = [db.protein(i)["consensus"] for i in range(len(Ks))]
    db.close()
    rng = np.random.default_rng(25)
    read = rng.integers(0, 4, size=3000).astype(np.uint8)
    planted = []
    at = 100
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
        for _ in range(19):
            a = int(rng.integers(0, 2300))
            wins.append((p, 0, a, a + int(rng.integers(30, 700))))
    got = []
    for load in ("dcp", "hmm"):
        with deciphon_amd.Engine(0) as eng:
            eng.load_dcp(dcp) if load == "dcp" else eng.load_hmm(hmm)
            eng.commit()
            eng.set_sequences([read])
            eng.set_mode(True, False)
            nul, alt = eng.cost(wins)
            paths = eng.path([wins[i] for i in hit_wins], trellis=False)
        got.append((nul, alt, paths))
    (nul_a, alt_a, paths_a), (nul_b, alt_b, paths_b) = got
    assert np.array_equal(nul_a.view(np.uint32), nul_b.view(np.uint32))
    assert np.array_equal(alt_a.view(np.uint32), alt_b.view(np.uint32))
    assert np.isfinite(alt_a[hit_wins]).all()
    for K, a, b in zip(Ks, paths_a, paths_b):
        assert bits(a["score"]) == bits(b["score"]), K
        assert len(a["state_ids"]) > 10, K
        assert np.array_equal(a["state_ids"], b["state_ids"]) and np.array_equal(a["seqsizes"], b["seqsizes"]), K


# ---- the scan -------------------------------------------------------------------------------------------

def consensus_batch():
    from deciphon_amd.scan import Batch, Sequence

    batch = Batch()
    for i, (_, s) in enumerate(read_fasta(os.path.join(GOLDEN, "consensus.fna"))):
        batch.add(Sequence(i, f"seq{i}", s))
    return batch


def open_paths():
    return {os.path.realpath(os.path.join("/proc/self/fd", f)) for f in os.listdir("/proc/self/fd")
            if os.path.exists(os.path.join("/proc/self/fd", f))}


@pytest.mark.parametrize("epsilon", [0.01, 0.1])
def test_scan_from_hmm_equals_the_scan_of_the_pressed_file(tmp_path, epsilon):
    from deciphon_amd.scan import Scan

    hmm = str(tmp_path / "minifam.hmm")
    with open(HMM) as f:
        (tmp_path / "minifam.hmm").write_text(f.read())
    dcp = press(hmm, str(tmp_path / "minifam.dcp"), 1, epsilon)
    batch = consensus_batch()
    with Scan(dcp, 0, 1, True, False, False) as scan:
        scan.run(str(tmp_path / "pressed"), batch)
        want = scan.products()
    os.unlink(dcp)
    with Scan.from_hmm(hmm, 1, epsilon) as scan:
        assert os.path.realpath(hmm) not in open_paths()  # the file was read and closed
        scan.run(str(tmp_path / "direct"), batch)
        rows = scan.products()
        stats, timing = scan.product_stats(), scan.last_timing()
    assert sorted(os.listdir(tmp_path)) == ["direct", "minifam.hmm", "pressed"]  # nothing written beside the .hmm
    assert rows == want and len(rows) == 3
    assert open(tmp_path / "direct" / "products.tsv").read() == open(tmp_path / "pressed" / "products.tsv").read()
    assert stats["rows"] == 3 and stats["file_bytes"] == os.path.getsize(tmp_path / "direct" / "products.tsv")
    assert timing["path_passes"] >= 3 and timing["total_s"] > 0
    if epsilon == 0.01:  # what the reference wrote at its default error rate
        gold = [ln.rstrip("\n").split("\t") for ln in open(os.path.join(GOLDEN, "products.tsv"))][1:]
        assert len(gold) == 3
        for got, ref in zip(rows, gold):
            g = got.split("\t")
            assert g[:10] == ref[:10]
            assert g[11] == ref[11]


def test_scan_from_hmm_of_three_positions(tmp_path):
    from deciphon_amd.scan import Batch, Scan, Sequence

    hmm = os.path.join(GOLDEN, "massive.hmm")
    dcp = press(hmm, str(tmp_path / "massive.dcp"))
    rng = np.random.default_rng(3)
    read = "".join(rng.choice(list("ACGT"), size=10000))
    batch = Batch()
    batch.add(Sequence(1, "seq1", read))
    with Scan(dcp, 0, 1, True, False, False) as scan:
        scan.run(str(tmp_path / "pressed"), batch)
        want = scan.products()
    with Scan.from_hmm(hmm) as scan:
        scan.run(str(tmp_path / "direct"), batch)
        assert scan.products() == want
    assert open(tmp_path / "direct" / "products.tsv").read() == open(tmp_path / "pressed" / "products.tsv").read()
