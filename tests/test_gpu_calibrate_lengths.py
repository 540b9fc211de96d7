"""GPU: the calibration over a ladder of read lengths (Engine.calibrate_lengths).  At a fixed lambda every rung has the
bits Engine.calibrate leaves for that rung's length and seed; with lambda fitted, lambda and every mu are held to the
float64 solver of tests/calib_ladder.py over the fp32 scores a plain cost pass gives for the same reads, replayed rung
by rung as tests/test_gpu_calibrate.py replays its one length.  Profiles, routes and helpers are that file's."""
import math
import os

import numpy as np
import pytest

import calib_ladder
from dcp_synth import random_protein
from dcp_testlib import GOLDEN, bits
from deciphon_amd import host
from test_gpu_calibrate import EFUNCUSE, FREQ, KS, assert_routes, ran, random_reads, refused, ulps, windows

pytestmark = pytest.mark.gpu

SEED, LAMBDA = 20262, 0.5
LENS = (30, 60, 120)
NSEQS = (1, 63, 64, 65, 200)
HMM = os.path.join(GOLDEN, "minifam.hmm")
NP = len(KS)


@pytest.fixture(scope="module")
def eng():
    """an engine of this module's own, with the three profiles of test_gpu_calibrate.py"""
    import deciphon_amd

    rng = np.random.default_rng(77)
    e = deciphon_amd.Engine(0)
    for p in [random_protein(rng, K, f"CAL{K}") for K in KS]:
        e.add_protein(p.core_size, p.trans, p.emission, p.BMk, p.null_emission, p.bg_emission)
    e.commit()
    e.set_mode(True, False)
    yield e
    e.close()


def replay_of(e, nprof, nseq, lens, seed, freq):
    """x[profile][rung][read], fp32 as dcp_lrt_filter_kernel forms it: the reads of rung j are those of seed + j, as
    plain reads"""
    x = np.zeros((nprof, len(lens), nseq), np.float32)
    for j, length in enumerate(lens):
        e.set_sequences(random_reads((seed + j) % 2**64, nseq, length, freq))
        nul, alt = e.cost(windows(nprof, nseq, length))
        with np.errstate(invalid="ignore"):
            x[:, j] = (np.float32(-2.0) * ((-nul) - (-alt))).astype(np.float32).reshape(nprof, nseq)
    return x


@pytest.fixture(scope="module")
def replay(eng):
    """of the 200 reads of every rung: read s does not depend on how many reads there are, so fewer are a prefix"""
    x = replay_of(eng, NP, max(NSEQS), LENS, SEED, FREQ)
    assert np.isfinite(x).all()
    x.setflags(write=False)
    return x


def state(e, nprof=NP):
    """everything a query answers, by the bits"""
    lens = e.calib_lengths
    return (lens, bits(e.calib_lambda),
            [(bits(e.profile_lambda(p)), bits(e.profile_mu(p)), e.profile_calib_excluded(p), bits(e.profile_mu_at(p, 77)),
              [(bits(e.profile_mu_rung(p, j)), e.profile_calib_excluded_rung(p, j)) for j in range(len(lens) + 1)])
             for p in range(nprof + 1)])


def assert_uncalibrated(e, nprof):
    assert e.calib_lengths == () and math.isnan(e.calib_lambda)
    for p in range(nprof):
        assert math.isnan(e.profile_lambda(p)) and math.isnan(e.profile_mu(p)) and math.isnan(e.profile_mu_rung(p, 0))
        assert math.isnan(e.profile_mu_at(p, 60)) and e.profile_calib_excluded(p) == 0 and e.profile_calib_excluded_rung(p, 0) == 0


# ---- 1. fixed lambda: rung by rung the single-length calibration ---------------------------------------------------

@pytest.mark.parametrize("rungs", [1, 2, 3])
@pytest.mark.parametrize("nseq", NSEQS)
def test_fixed_lambda_has_the_bits_of_calibrate(eng, nseq, rungs):
    lens = LENS[:rungs]
    eng.calibrate_lengths(nseq, lens, SEED, FREQ, LAMBDA)
    assert eng.calib_lengths == lens and eng.calib_lambda == LAMBDA
    # the reads of the last rung stay resident
    assert eng.num_sequences == nseq
    reads = random_reads(SEED + rungs - 1, nseq, lens[-1], FREQ)
    for s in {0, nseq // 2, nseq - 1}:
        assert np.array_equal(eng.code_rows(s), host.code_rows_of(reads[s])), s
    got = [[(bits(eng.profile_mu_rung(p, j)), eng.profile_calib_excluded_rung(p, j)) for j in range(rungs)] for p in range(NP)]
    assert all(eng.profile_lambda(p) == np.float32(LAMBDA) for p in range(NP))
    assert [bits(eng.profile_mu(p)) for p in range(NP)] == [got[p][0][0] for p in range(NP)]  # the old query: rung 0
    assert all(math.isnan(eng.profile_mu_rung(p, rungs)) for p in range(NP))
    for j, length in enumerate(lens):
        eng.calibrate(nseq, length, SEED + j, FREQ, LAMBDA)
        for p in range(NP):
            assert got[p][j] == (bits(eng.profile_mu(p)), eng.profile_calib_excluded(p)), (KS[p], length)
            assert np.isfinite(eng.profile_mu(p))


# ---- 2. fitted lambda against the float64 solver -----------------------------------------------------------------------

@pytest.mark.parametrize("nseq", (2, 63, 64, 65, 200))
def test_fitted_lambda_is_the_solvers(eng, replay, nseq):
    eng.calibrate_lengths(nseq, LENS, SEED, FREQ, 0.0)
    assert_routes(eng)
    assert eng.calib_lambda == 0.0 and eng.calib_lengths == LENS
    for p in range(NP):
        lam, mu = calib_ladder.fit(replay[p, :, :nseq])
        got = eng.profile_lambda(p)
        print(f"K = {KS[p]}, nseq = {nseq}: lambda {got!r}, solver {lam!r}, {ulps(got, np.float32(lam))} ulp")
        assert ulps(got, np.float32(lam)) <= 2, (KS[p], nseq, got, lam)
        for j in range(len(LENS)):
            m = eng.profile_mu_rung(p, j)
            print(f"    rung {LENS[j]}: mu {m!r}, solver {mu[j]!r}, {ulps(m, np.float32(mu[j]))} ulp")
            assert ulps(m, np.float32(mu[j])) <= 2, (KS[p], nseq, j, m, mu[j])
            assert eng.profile_calib_excluded_rung(p, j) == 0


def test_fixed_lambda_is_the_closed_form(eng, replay):
    """the ladder at a fixed lambda against numpy as well, not only against calibrate()"""
    eng.calibrate_lengths(200, LENS, SEED, FREQ, LAMBDA)
    for p in range(NP):
        _, mu = calib_ladder.fit(replay[p], float(np.float32(LAMBDA)))
        for j in range(len(LENS)):
            assert ulps(eng.profile_mu_rung(p, j), np.float32(mu[j])) <= 2


# ---- 3. mu at a window length ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lam", [LAMBDA, 0.0], ids=["fixed", "fitted"])
def test_profile_mu_at_is_the_hosts_rule(eng, lam):
    eng.calibrate_lengths(64, LENS, SEED, FREQ, lam)
    for p in range(NP):
        mu = [eng.profile_mu_rung(p, j) for j in range(len(LENS))]
        assert np.isfinite(mu).all()
        for length in (60, 45, 100, 7, 1000):
            assert eng.profile_mu_at(p, length) == host.calib_mu_at(LENS, mu, length), (KS[p], length)
        assert eng.profile_mu_at(p, 60) == float(mu[1])
        assert math.isnan(eng.profile_mu_at(p, 0))
    assert math.isnan(eng.profile_mu_at(NP, 60)) and math.isnan(eng.profile_mu_at(-1, 60))


# ---- 4. equal reads, excluded scores ---------------------------------------------------------------------------------------

def test_equal_reads(eng):
    """freq = [1, 0, 0, 0]: every read is poly-A, every score of a rung the same"""
    only_a = [1, 0, 0, 0]
    x = replay_of(eng, NP, 8, LENS, SEED, only_a)
    assert np.isfinite(x).all() and (x == x[:, :, :1]).all()
    eng.calibrate_lengths(8, LENS, SEED, only_a, 0.0)
    for p in range(NP):
        assert math.isnan(eng.profile_lambda(p))
        for j in range(len(LENS)):
            assert math.isnan(eng.profile_mu_rung(p, j)) and eng.profile_calib_excluded_rung(p, j) == 0
        assert math.isnan(eng.profile_mu_at(p, 60))
    assert eng.calib_lambda == 0.0 and eng.calib_lengths == LENS
    eng.calibrate_lengths(8, LENS, SEED, only_a, LAMBDA)
    for p in range(NP):
        for j in range(len(LENS)):
            assert bits(eng.profile_mu_rung(p, j)) == bits(x[p, j, 0]), (KS[p], j)  # log(n / n) = 0: the common score


def test_excluded_scores_and_unequal_counts():
    """minifam.hmm at epsilon 0: a read whose length is no multiple of 3 scores +inf under both models (DESIGN.md section
    2), so rung 31 is left out whole, and rungs 30 and 60 lose what the replay shows as not finite"""
    import deciphon_amd

    lens, nseq = (30, 31, 60), 64
    with deciphon_amd.Engine(0) as e:
        e.load_hmm(HMM, 1, 0.0)
        e.commit()
        e.set_mode(True, False)
        n = e.num_profiles
        x = replay_of(e, n, nseq, lens, SEED, FREQ)
        finite = np.isfinite(x)
        assert not finite[:, 1].any()
        for p in range(n):  # the precondition: some rung keeps two distinct scores
            assert any(len(set(x[p, j][finite[p, j]].tolist())) >= 2 for j in (0, 2)), p
        e.calibrate_lengths(nseq, lens, SEED, FREQ, 0.0)
        for p in range(n):
            lam, mu = calib_ladder.fit(x[p])
            assert [e.profile_calib_excluded_rung(p, j) for j in range(3)] == [int((~finite[p, j]).sum()) for j in range(3)]
            assert e.profile_calib_excluded_rung(p, 1) == nseq and math.isnan(e.profile_mu_rung(p, 1))
            print(f"profile {p}: excluded {[e.profile_calib_excluded_rung(p, j) for j in range(3)]}, lambda {e.profile_lambda(p)!r}, "
                  f"solver {lam!r}")
            assert ulps(e.profile_lambda(p), np.float32(lam)) <= 2
            got = [e.profile_mu_rung(p, j) for j in range(3)]
            for j in (0, 2):
                if math.isnan(mu[j]):
                    assert math.isnan(got[j])
                else:
                    assert ulps(got[j], np.float32(mu[j])) <= 2, (p, j, got[j], mu[j])
            assert e.profile_mu_at(p, 40) == host.calib_mu_at(lens, got, 40)
            if np.isfinite([got[0], got[2]]).all():  # rung 31 is bridged: the line through rungs 30 and 60
                want = float(got[0]) + (float(got[2]) - float(got[0])) * math.log(40 / 30) / math.log(60 / 30)
                assert abs(e.profile_mu_at(p, 40) - want) <= 1e-12 * max(1.0, abs(want))


# ---- 5. chunks --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lam", [LAMBDA, 0.0], ids=["fixed", "fitted"])
def test_chunk_edges(eng, monkeypatch, lam):
    """65 windows per chunk: three profiles x 65 reads take three chunks per rung (130: two; 1: a profile is never split)"""
    monkeypatch.delenv("DECIPHON_HIP_CALIB_WINDOWS", raising=False)
    eng.calibrate_lengths(65, LENS, SEED, FREQ, lam)
    assert len(ran(eng.last_cost_launches())) == 3
    one = state(eng)
    for cap in ("65", "1", "130"):
        monkeypatch.setenv("DECIPHON_HIP_CALIB_WINDOWS", cap)
        eng.calibrate_lengths(65, LENS, SEED, FREQ, lam)
        assert len(ran(eng.last_cost_launches())) == 1, cap  # the last chunk is the last profile alone
        assert state(eng) == one, cap


# ---- 6. contract ------------------------------------------------------------------------------------------------------

def test_refused_while_a_batch_is_outstanding(eng):
    eng.calibrate_lengths(8, LENS, SEED, FREQ, 0.0)
    before = state(eng)
    eng.set_sequences(random_reads(99, 4, 30))
    rows = eng.code_rows(2)
    eng.cost_hits_begin(windows(NP, 4, 30))
    try:
        assert refused(eng.calibrate_lengths, 5, (10, 20), SEED, None, LAMBDA)
        assert eng.num_sequences == 4 and np.array_equal(eng.code_rows(2), rows)
        assert state(eng) == before
    finally:
        eng.cost_hits_end()
    eng.calibrate_lengths(5, (10, 20), SEED, None, LAMBDA)
    assert eng.calib_lengths == (10, 20) and eng.num_sequences == 5


def test_bad_arguments_change_nothing(eng):
    eng.calibrate_lengths(8, LENS, SEED, FREQ, 0.0)
    before = state(eng)
    eng.set_sequences(random_reads(99, 4, 30))
    rows = eng.code_rows(3)
    for lens in ((), tuple(range(1, 18)), (0, 30), (-3, 30), (60, 30), (30, 30), (30, 60, 60)):
        assert refused(eng.calibrate_lengths, 8, lens, SEED, FREQ, LAMBDA), lens
    assert eng.lib.dcp_hip_calibrate_lengths(eng.h, 8, 2, None, SEED, None, LAMBDA) == EFUNCUSE
    for lam in (-0.5, float("nan"), float("inf"), float("-inf")):
        assert refused(eng.calibrate_lengths, 8, LENS, SEED, FREQ, lam), lam
    assert refused(eng.calibrate_lengths, 1, LENS, SEED, FREQ, 0.0)  # a scale from one score
    for nseq in (0, -1):
        assert refused(eng.calibrate_lengths, nseq, LENS, SEED, FREQ, LAMBDA)
    for freq in ([-1, 1, 1, 1], [float("nan"), 1, 1, 1], [0, 0, 0, 0]):
        assert refused(eng.calibrate_lengths, 8, LENS, SEED, freq, LAMBDA)
    # code rows beyond 2^32 at the second rung alone: refused before the first is installed
    assert refused(eng.calibrate_lengths, 70000, (30, 70000), SEED, FREQ, LAMBDA)
    assert eng.num_sequences == 4 and np.array_equal(eng.code_rows(3), rows)
    assert state(eng) == before
    eng.calibrate_lengths(2, tuple(range(1, 17)), SEED, FREQ, LAMBDA)  # DCP_CALIB_MAX_LENS rungs are taken
    assert eng.calib_lengths == tuple(range(1, 17))


def test_seeds(eng):
    eng.calibrate_lengths(64, LENS, SEED, FREQ, 0.0)
    first, rows = state(eng), eng.code_rows(63)
    eng.calibrate_lengths(64, LENS, SEED, FREQ, 0.0)
    assert state(eng) == first and np.array_equal(eng.code_rows(63), rows)
    eng.calibrate_lengths(64, LENS, SEED + 1, FREQ, 0.0)
    assert state(eng) != first and not np.array_equal(eng.code_rows(63), rows)
    # rung j of SEED + 1 is rung j + 1 of SEED where the lengths agree ...
    eng.calibrate_lengths(64, (60,), SEED + 1, FREQ, LAMBDA)
    mu = [bits(eng.profile_mu_rung(p, 0)) for p in range(NP)]
    eng.calibrate_lengths(64, (30, 60), SEED, FREQ, LAMBDA)
    assert [bits(eng.profile_mu_rung(p, 1)) for p in range(NP)] == mu
    # ... and seed + j wraps at 2^64
    eng.calibrate_lengths(64, (30, 60), 2**64 - 1, FREQ, LAMBDA)
    wrapped = [bits(eng.profile_mu_rung(p, 1)) for p in range(NP)]
    eng.calibrate(64, 60, 0, FREQ, LAMBDA)
    assert [bits(eng.profile_mu(p)) for p in range(NP)] == wrapped


def test_calibrate_leaves_a_ladder_of_one_rung(eng):
    eng.calibrate_lengths(16, LENS, SEED, FREQ, 0.0)
    eng.calibrate(16, 60, SEED, FREQ, LAMBDA)
    assert eng.calib_lengths == (60,) and eng.calib_lambda == LAMBDA
    for p in range(NP):
        mu = eng.profile_mu(p)
        assert np.isfinite(mu) and eng.profile_lambda(p) == np.float32(LAMBDA)
        assert bits(eng.profile_mu_rung(p, 0)) == bits(mu) and math.isnan(eng.profile_mu_rung(p, 1))
        for length in (1, 59, 60, 61, 10**6):
            assert eng.profile_mu_at(p, length) == float(mu)


def test_gone_after_what_changes_a_score():
    """on profiles from a HMMER3 file: dcp_hip_set_epsilon and _set_gencode work only on those"""
    import deciphon_amd

    with deciphon_amd.Engine(0) as e:
        assert_uncalibrated(e, 1)
        e.calibrate_lengths(8, (30, 60), SEED)  # no profiles: the sequences of the last rung are set, and that is all
        assert e.num_sequences == 8 and len(e.code_rows(0)) == 61
        assert_uncalibrated(e, 1)
        e.load_hmm(HMM, 1, 0.01)
        e.commit()
        n = e.num_profiles
        assert refused(e.calibrate_lengths, 8, (30, 60), SEED, None, 0.0)  # no mode yet
        e.set_mode(True, False)

        def calibrated():
            e.calibrate_lengths(16, (30, 60), SEED, None, 0.0)
            assert e.calib_lengths == (30, 60) and e.calib_lambda == 0.0
            assert all(np.isfinite(e.profile_lambda(p)) and np.isfinite(e.profile_mu_at(p, 45)) for p in range(n))
            return state(e, n)

        base = calibrated()
        e.set_epsilon(0.02)
        assert_uncalibrated(e, n)
        assert calibrated() != base
        e.set_epsilon(0.01)
        assert_uncalibrated(e, n)
        assert calibrated() == base
        e.set_gencode(11)
        assert_uncalibrated(e, n)
        calibrated()
        e.set_gencode(1)
        e.set_mode(False, False)
        assert_uncalibrated(e, n)
        assert calibrated() != base
        e.set_mode(True, False)
        assert_uncalibrated(e, n)
        assert calibrated() == base
        e.set_xtrans_table(np.zeros((0, 13), np.float32))
        assert_uncalibrated(e, n)
        assert calibrated() == base
        # profiles added later have none; the others keep theirs
        e.load_hmm(HMM, 1, 0.01, 0, 1)
        e.commit()
        assert state(e, n)[2][:n] == base[2][:n]
        assert math.isnan(e.profile_lambda(n)) and math.isnan(e.profile_mu_at(n, 45)) and math.isnan(e.profile_mu_rung(n, 0))
        e.clear_profiles()
        assert_uncalibrated(e, n)
