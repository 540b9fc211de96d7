"""GPU: press and scan away from the default error rate.

Press: every entry of every table (nodes 0..K, null and background of every profile, all 1364 codes) of databases
pressed at epsilon from 0 to 1 -- the smallest fp32 subnormal included, where e^2 underflows fp32 -- against the
quasi-codon model in float64 (dcp_testlib.emission_probs): -inf exactly where the model is 0, elsewhere within
2e-5 max(1, |x|), the bound tests/test_decoder.py pins the model to the reference's pressed tables with.

Scan: databases pressed at epsilon = 0, 0.1 and 1e-30, scored by every family of cost kernel and the fast path
pass, bit for bit against the CPU oracle; the device lrt filter on windows whose lrt is -inf, +inf and NaN (at
epsilon = 0 a window whose length is not a multiple of 3 has null = alt = +inf); dcp_scan_run's rows against the
oracle scan, decoded codons included."""
import numpy as np
import pytest

import dcp_testlib
from dcp_testlib import bits
from hmm_testlib import HMM, star_profile, without_stops  # table 1's stops: the T of TAA, TAG and TGA becomes a C

pytestmark = pytest.mark.gpu

EPSILONS = (0.0, 1.4e-45, 1e-38, 1e-30, 1e-22, 1e-20, 1e-19, 1e-12, 1e-4, 0.01, 0.1, 0.5, 0.999, 1.0)


def press(hmm, out, epsilon):
    from deciphon_amd import Press

    with Press(hmm, out, 1, epsilon) as p:
        while not p.end():
            p.next()


@pytest.fixture(scope="module")
def press_hmm(tmp_path_factory):
    """K = 1, 2, 3, 300 and 4100; a profile with zero-probability (*) match emissions, so that codon marginals of
    whole amino acids are 0; and one whose match emissions are almost one-hot (every other amino acid at e^-60),
    for the smallest non-zero marginals."""
    from deciphon_amd import synth

    seeds = synth.load_hmm_seeds(HMM)
    profiles = list(synth.pfam_like_hmms(seeds, 5, 23, lengths=[1, 2, 3, 300, 4100]))
    rng = np.random.default_rng(5)
    star = star_profile(seeds, rng)
    onehot = synth.resample_hmm(seeds, 40, rng, "ONEHOT0.1")
    for k, nd in enumerate(onehot["nodes"]):
        nd["match"] = ["0.00000" if j == k % 20 else "60.00000" for j in range(20)]
    path = str(tmp_path_factory.mktemp("eps") / "press.hmm")
    synth.write_hmm(path, profiles + [star, onehot])
    return path


@pytest.mark.parametrize("epsilon", EPSILONS)
def test_kernel_equals_the_model_on_every_entry(press_hmm, tmp_path, epsilon):
    from deciphon_amd.host import Database

    e32 = np.float32(epsilon)
    out = str(tmp_path / "eps.dcp")
    press(press_hmm, out, float(e32))
    db = Database(out)
    assert db.epsilon == e32 and len(db) == 7
    saw_zero = saw_star = False
    for i in range(len(db)):
        p = db.protein(i)
        K = p["core_size"]
        got = np.concatenate([p["null_emission"][None], p["bg_emission"][None], p["emission"]]).astype(np.float64)
        assert got.shape == (K + 3, 1364) and p["nucltp"].shape == (K + 3, 4)
        want = dcp_testlib.emission_probs(float(e32), p["nucltp"], p["codonm"])
        zero = want == 0.0
        saw_zero |= bool(zero.any())
        saw_star |= bool(np.isneginf(p["codonm"]).sum() > 3 * len(p["codonm"]))  # more than the stop codons
        where = f"protein {i} (K = {K}) at epsilon {e32!r}"
        assert not np.isnan(got).any() and not np.isposinf(got).any(), where
        wrong_inf = np.isneginf(got) != zero
        assert not wrong_inf.any(), (f"{where}: {int(wrong_inf.sum())} entries -inf where the model is not 0 or the "
                                     f"reverse, first (row, code) {tuple(int(v) for v in np.argwhere(wrong_inf)[0])}")
        lw = np.log(want[~zero])
        err = np.abs(got[~zero] - lw) / np.maximum(1.0, np.abs(lw))
        worst = int(np.argmax(err))
        assert err[worst] <= 2e-5, f"{where}: relative log error {err[worst]:.3g} at log P = {lw[worst]:.6g}"
    db.close()
    if epsilon in (0.0, 1.0):
        assert saw_zero  # e = 0 and e = 1 leave whole code lengths at probability 0
    assert saw_star


# ---- databases pressed at other error rates, scored against the oracle --------------------------------------------


# a pack shape (7, 60, 100), one wave (200), the narrow 384 and 768 layouts (300, 600), multi-wave (1500), strip (4200)
SCAN_KS = (7, 60, 100, 200, 300, 600, 1500, 4200)
READ = 1202


@pytest.fixture(scope="module")
def pressed(tmp_path_factory):
    """{epsilon: (path, proteins)} of SCAN_KS pressed at epsilon 0, 0.1 and 1e-30, and one read per profile carrying
    a planted, error-bearing copy of its consensus."""
    from deciphon_amd import synth
    from oracle.dcp_reader import read_dcp

    seeds = synth.load_hmm_seeds(HMM)
    d = tmp_path_factory.mktemp("eps_scan")
    hmm = str(d / "scan.hmm")
    synth.write_hmm(hmm, synth.pfam_like_hmms(seeds, len(SCAN_KS), 31, lengths=list(SCAN_KS)))
    dbs = {}
    for eps in (0.0, 0.1, 1e-30):
        out = str(d / f"scan_{eps}.dcp")
        press(hmm, out, float(np.float32(eps)))
        dbs[eps] = (out, read_dcp(out).proteins)
    rng = np.random.default_rng(12)
    reads = []
    for p in dbs[0.1][1]:
        x = rng.integers(0, 4, size=READ).astype(np.uint8)
        a = int(rng.integers(0, max(len(p.consensus) - 150, 1)))
        dom = synth.mutate(synth.back_translate(p.consensus[a : a + 150]), rng, 0.05, 0.01, 0.01)[:900]
        x[150 : 150 + len(dom)] = dom
        reads.append(without_stops(x))
    return dbs, reads


def _windows(n):
    """per profile: lengths 1..5, 31..33 and 300..302 from inside the planted domain, and the whole read minus 0, 1
    and 2 nucleotides -- every residue mod 3"""
    w = []
    for i in range(n):
        w += [(i, i, 160, 160 + L) for L in (1, 2, 3, 4, 5, 31, 32, 33, 300, 301, 302)]
        w += [(i, i, 0, READ - r) for r in (0, 1, 2)]
    return w


@pytest.mark.parametrize("eps", [0.0, 0.1, 1e-30])
def test_engine_on_pressed_tables_equals_the_oracle(pressed, orc, monkeypatch, eps):
    import deciphon_amd

    dbs, reads = pressed
    path, proteins = dbs[eps]
    profs = [orc.setup_profile(p) for p in proteins]
    wins = _windows(len(proteins))
    with deciphon_amd.Engine(0) as eng:
        eng.load_dcp(path)
        eng.commit()
        assert [eng.core_size(i) for i in range(len(proteins))] == list(SCAN_KS)
        eng.set_sequences(reads)
        eng.set_mode(True, False)
        monkeypatch.delenv("DECIPHON_HIP_PACK_LDS", raising=False)
        nul, alt = eng.cost(wins)
        monkeypatch.setenv("DECIPHON_HIP_PACK_LDS", "0")
        nul2, alt2 = eng.cost(wins)
        monkeypatch.delenv("DECIPHON_HIP_PACK_LDS")
        assert np.array_equal(nul.view(np.uint32), nul2.view(np.uint32))
        assert np.array_equal(alt.view(np.uint32), alt2.view(np.uint32))
        finite = []
        for i, (pi, si, a, b) in enumerate(wins):
            seq = np.ascontiguousarray(reads[si][a:b])
            xt = orc.xtrans(max((b - a) // 3, 1), True, False)
            want_nul, want_alt = orc.null(profs[pi], xt, seq), orc.cost(profs[pi], xt, seq)
            assert bits(nul[i]) == bits(want_nul), (eps, SCAN_KS[pi], b - a)
            assert bits(alt[i]) == bits(want_alt), (eps, SCAN_KS[pi], b - a)
            if eps == 0.0:  # every step emits a whole codon
                assert np.isfinite(want_nul) == np.isfinite(want_alt) == ((b - a) % 3 == 0), (SCAN_KS[pi], b - a)
            if np.isfinite(want_alt):
                finite.append(i)
        assert len(finite) >= 4 * len(proteins)  # lengths 3, 33, 300 and the whole read at least
        # the fast path pass on every window with a path (+inf windows have none to trace)
        pw = [wins[i] for i in finite]
        res = eng.path(pw, trellis=False)
        assert 0 <= eng.path_redone <= len(pw)
        for (pi, si, a, b), r in zip(pw, res):
            seq = np.ascontiguousarray(reads[si][a:b])
            xt = orc.xtrans(max((b - a) // 3, 1), True, False)
            score, xo, no = orc.path(profs[pi], xt, seq)
            ids, sizes = orc.unzip(profs[pi].K, len(seq), xo, no)
            assert bits(r["score"]) == bits(score), (eps, SCAN_KS[pi], b - a)
            assert np.array_equal(r["state_ids"], ids) and np.array_equal(r["seqsizes"], sizes), (eps, SCAN_KS[pi], b - a)
            if eps == 0.0:
                assert set(r["seqsizes"].tolist()) <= {0, 3}


def test_device_filter_drops_nan_and_infinite_lrt(pressed, orc):
    """One cost_hits call over windows whose lrt is -inf (a profile with no way into its core), +inf (a profile whose
    null model emits nothing: null = +inf, alt finite), NaN (epsilon = 0, length not a multiple of 3) and finite:
    the kept windows and lrt bits are those of the host filter isfinite(lrt) && lrt >= 0 on cost()'s scores."""
    import deciphon_amd
    from deciphon_amd import host

    dbs, reads = pressed
    path, proteins = dbs[0.0]
    rng = np.random.default_rng(44)
    closed = dcp_testlib.synth_profile(rng, 40)
    closed.trans[0, :] = np.float32(np.inf)
    silent = dcp_testlib.synth_profile(rng, 50)
    silent.null[:] = np.float32(np.inf)
    with deciphon_amd.Engine(0) as eng:
        eng.load_dcp(path)
        for p in (closed, silent):
            eng.add_profile(p.K, p.trans, p.match, p.null, p.bg)
        eng.commit()
        eng.set_sequences(reads)
        eng.set_mode(True, False)
        n = len(proteins)
        wins = _windows(n) + [(q, s, 0, READ - r) for q in (n, n + 1) for s in range(0, n, 3) for r in (0, 1)]
        wins = np.array(wins, np.int32)
        nul, alt = eng.cost(wins)
        lrt = np.array([host.lrt(-a, -b) for a, b in zip(nul, alt)], np.float32)
        assert np.isnan(lrt).any() and np.isposinf(lrt).any() and np.isneginf(lrt).any()
        keep = np.nonzero(np.isfinite(lrt) & (lrt >= 0))[0]
        assert len(keep) > 0
        idx, got = eng.cost_hits(wins)
        assert np.array_equal(idx, keep.astype(np.int32))
        assert np.array_equal(got.view(np.uint32), lrt[keep].view(np.uint32))


@pytest.mark.parametrize("mode", [(True, False), (False, True)])
@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_scan_of_pressed_database_equals_the_oracle_scan(tmp_path, orc, eps, mode):
    """dcp_scan_run on a database pressed at eps: its rows -- windows, lrt, paths, and codons and amino acids decoded
    at eps -- equal the oracle scan's."""
    from deciphon_amd import synth
    from deciphon_amd.scan import Batch, Scan, Sequence
    from oracle.dcp_reader import read_dcp

    seeds = synth.load_hmm_seeds(HMM)
    hmm, out = str(tmp_path / "s.hmm"), str(tmp_path / "s.dcp")
    synth.write_hmm(hmm, synth.pfam_like_hmms(seeds, 3, 57, lengths=[40, 173, 320]))
    press(hmm, out, float(np.float32(eps)))
    proteins = read_dcp(out).proteins
    # every read planted; lengths 1400, 1399, 1398: one window each, of every residue mod 3 (only 1398 scores at 0)
    raw = synth.synth_reads(12, 1400, [p.consensus for p in proteins], 91, planted_every=1, sub=0.05, ins=0.01,
                            dele=0.01)
    reads = [(i + 1, "".join("ACGT"[v] for v in without_stops(r[: 1400 - i % 3]))) for i, r in enumerate(raw)]
    batch = Batch()
    for sid, text in reads:
        batch.add(Sequence(sid, f"r{sid}", text))
    with Scan(out, 0, 1, mode[0], mode[1], False) as scan:
        scan.run(str(tmp_path / "prod"), batch)
        rows = scan.products()
    want = dcp_testlib.oracle_scan(orc, proteins, reads, mode[0], mode[1], epsilon=float(np.float32(eps)))
    assert len(want) > 0
    assert rows == want
