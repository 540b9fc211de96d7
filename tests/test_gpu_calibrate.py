"""GPU: random reads whose code rows the device writes (Engine.set_random_sequences) and the calibration of profiles on
them (Engine.calibrate), against the host's statement of the same reads (host.random_nt, host.code_rows_of) and a numpy
float64 fit of the fp32 scores a plain cost pass gives over them.

Profiles come from tests/dcp_synth.py, one core size per route of the cost pass: K = 12 (a pack shape), 173 (one
wavefront), 700 (two wavefronts).  The engine's own report of its launches says that each ran."""
import math
import os

import numpy as np
import pytest

from dcp_synth import random_protein
from dcp_testlib import GOLDEN, bits
from deciphon_amd import host
from deciphon_amd.hip import HipError

pytestmark = pytest.mark.gpu

KS = (12, 173, 700)
SEED, LEN, LAMBDA = 20261, 60, 0.5
FREQ = [0.2, 0.3, 0.3, 0.2]
NSEQS = (1, 63, 64, 65, 200)
HMM = os.path.join(GOLDEN, "minifam.hmm")
EFUNCUSE = 8


def random_reads(seed, nseq, length, freq=None):
    nt = host.random_nt(seed, nseq * length, 0, freq)
    return [np.ascontiguousarray(nt[s * length:(s + 1) * length]) for s in range(nseq)]


def windows(nprof, nseq, length):
    return np.array([(p, s, 0, length) for p in range(nprof) for s in range(nseq)], np.int32)


def mu_of(nul, alt, lam):
    """the fit in float64, from fp32 scores: x as dcp_lrt_filter_kernel forms it"""
    x = (np.float32(-2.0) * ((-nul) - (-alt))).astype(np.float32)
    assert np.isfinite(x).all()
    x = x.astype(np.float64)
    m = x.min()
    return m - math.log(np.exp(-float(np.float32(lam)) * (x - m)).mean()) / float(np.float32(lam))


def ulps(a, b):
    a, b = np.float32(a), np.float32(b)
    assert np.isfinite(a) and np.isfinite(b) and (a >= 0) == (b >= 0), (a, b)
    return abs(int(a.view(np.uint32)) - int(b.view(np.uint32)))


def ran(launches):
    """(kernel, index) of the launches that held windows"""
    return {(e["kernel"], e["index"]) for e in launches if e["count"] > 0 and e["kernel"] != "none"}


def assert_routes(eng):
    got = ran(eng.last_cost_launches())
    shape = host.engine_core_size(12)[4]
    assert ("pack_lds", shape) in got or ("pack", shape) in got, got
    assert ("class", host.engine_core_size(173)[2]) in got, got
    assert ("class", host.engine_core_size(700)[2]) in got, got


@pytest.fixture(scope="module")
def proteins():
    rng = np.random.default_rng(77)
    return [random_protein(rng, K, f"CAL{K}") for K in KS]


@pytest.fixture(scope="module")
def eng(proteins):
    """an engine of this module's own, so that nothing it sets reaches the other suites"""
    import deciphon_amd

    e = deciphon_amd.Engine(0)
    for p in proteins:
        e.add_protein(p.core_size, p.trans, p.emission, p.BMk, p.null_emission, p.bg_emission)
    e.commit()
    e.set_mode(True, False)
    yield e
    e.close()


@pytest.fixture(scope="module")
def oracle_scores(orc, proteins):
    """(null, alt) words of the oracle for every profile x every one of the 200 reads: the smaller sets are prefixes"""
    reads = random_reads(SEED, max(NSEQS), LEN, FREQ)
    xt = orc.xtrans(max(LEN // 3, 1), True, False)
    out = np.zeros((len(KS), len(reads), 2), np.float32)
    for i, p in enumerate(proteins):
        prof = orc.setup_profile(p)
        for s, r in enumerate(reads):
            out[i, s] = (orc.null(prof, xt, r), orc.cost(prof, xt, r))
    return out


# ---- 1. rows ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("length", [1, 4, 5, 6, 61])
@pytest.mark.parametrize("freq", [None, FREQ], ids=["uniform", "skewed"])
def test_rows_are_the_hosts(eng, length, freq):
    eng.set_random_sequences(5, length, SEED, freq)
    assert eng.num_sequences == 5
    for s, read in enumerate(random_reads(SEED, 5, length, freq)):
        assert np.array_equal(eng.code_rows(s), host.code_rows_of(read)), (length, s)


def test_rows_beyond_the_grid_stride(eng):
    """70000 sequences: more than gridDim.y holds, so blocks take several sequences each"""
    import ctypes as C

    nseq, length = 70000, 3
    eng.set_random_sequences(nseq, length, SEED, FREQ)
    assert eng.num_sequences == nseq
    got = np.zeros((nseq, length + 1, 8), np.uint32)
    for s in range(nseq):
        rc = eng.lib.dcp_hip_code_rows_read(eng.h, s, C.c_void_p(got.ctypes.data + s * got[0].nbytes), length + 1)
        assert rc == 0, s
    nt = host.random_nt(SEED, nseq * length, 0, FREQ).reshape(nseq, length).astype(np.uint32)
    want = np.zeros_like(got)
    off = (0, 4, 20)
    for r in range(1, length + 1):
        code = np.zeros(nseq, np.uint32)
        for t in range(1, r + 1):  # the t-mer ending at r: its leftmost symbol is the most significant digit
            code = code + (nt[:, r - t] << np.uint32(2 * (t - 1)))
            want[:, r, t - 1] = off[t - 1] + code
    for s in (0, 1, 65534, 65535, 65536, nseq - 1):  # the vectorised statement above, against the host's
        assert np.array_equal(want[s], host.code_rows_of(nt[s].astype(np.uint8))), s
    bad = np.nonzero((got != want).any(axis=(1, 2)))[0]
    assert len(bad) == 0, (len(bad), bad[:5].tolist())


def test_empty_inputs(eng):
    eng.set_random_sequences(0, 7, SEED)
    assert eng.num_sequences == 0
    nul, alt = eng.cost(np.zeros((0, 4), np.int32))
    assert len(nul) == 0 and len(alt) == 0
    eng.set_random_sequences(3, 0, SEED)
    assert eng.num_sequences == 3
    for s in range(3):
        assert np.array_equal(eng.code_rows(s), np.zeros((1, 8), np.uint32))
    eng.set_random_sequences(0, 0, SEED)
    assert eng.num_sequences == 0


# ---- 2. scores ----------------------------------------------------------------------------------------------

def test_oracle_scores_are_finite(oracle_scores):
    assert np.isfinite(oracle_scores).all()


@pytest.mark.parametrize("nseq", NSEQS)
def test_mu_is_the_fit_of_the_scores(eng, oracle_scores, nseq):
    assert np.isfinite(oracle_scores[:, :nseq]).all()
    eng.calibrate(nseq, LEN, SEED, FREQ, LAMBDA)
    assert_routes(eng)
    assert eng.num_sequences == nseq  # the random sequences stay resident
    mu = [eng.profile_mu(p) for p in range(len(KS))]
    assert [eng.profile_calib_excluded(p) for p in range(len(KS))] == [0, 0, 0]
    assert eng.calib_lambda == LAMBDA
    # the same reads as plain reads, the same windows
    eng.set_sequences(random_reads(SEED, nseq, LEN, FREQ))
    nul, alt = eng.cost(windows(len(KS), nseq, LEN))
    got = np.stack([nul, alt], axis=1).view(np.uint32).reshape(len(KS), nseq, 2)
    assert np.array_equal(got, oracle_scores[:, :nseq].view(np.uint32)), "the cost pass over these reads is not the oracle's"
    for p in range(len(KS)):
        want = np.float32(mu_of(nul[p * nseq:(p + 1) * nseq], alt[p * nseq:(p + 1) * nseq], LAMBDA))
        print(f"K = {KS[p]}, nseq = {nseq}: mu {mu[p]!r}, numpy {want!r}, {ulps(mu[p], want)} ulp")
        assert ulps(mu[p], want) <= 2, (KS[p], nseq, mu[p], want)
    for p in range(len(KS)):  # set_sequences and cost leave the calibration in force
        assert bits(eng.profile_mu(p)) == bits(mu[p])


# ---- 3. chunks ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cap", ["65", "1", "130"])
def test_chunk_edges_between_profiles(eng, monkeypatch, cap):
    """65 windows per chunk: three profiles x 65 reads take three chunks (130: two; 1: a profile is never split)"""
    monkeypatch.delenv("DECIPHON_HIP_CALIB_WINDOWS", raising=False)
    eng.calibrate(65, LEN, SEED, FREQ, LAMBDA)
    assert len(ran(eng.last_cost_launches())) == 3
    one = [bits(eng.profile_mu(p)) for p in range(len(KS))]
    monkeypatch.setenv("DECIPHON_HIP_CALIB_WINDOWS", cap)
    eng.calibrate(65, LEN, SEED, FREQ, LAMBDA)
    assert len(ran(eng.last_cost_launches())) == 1  # the last chunk is the last profile alone
    assert [bits(eng.profile_mu(p)) for p in range(len(KS))] == one
    assert [eng.profile_calib_excluded(p) for p in range(len(KS))] == [0, 0, 0]


# ---- 4. contract --------------------------------------------------------------------------------------------

def refused(call, *args):
    with pytest.raises(HipError) as e:
        call(*args)
    assert e.value.code == EFUNCUSE, e.value
    return True


def test_refused_while_a_batch_is_outstanding(eng):
    reads = random_reads(99, 4, 30)
    eng.calibrate(8, LEN, SEED, FREQ, LAMBDA)
    mu = [bits(eng.profile_mu(p)) for p in range(len(KS))]
    eng.set_sequences(reads)
    rows = eng.code_rows(2)
    eng.cost_hits_begin(windows(len(KS), 4, 30))
    try:
        assert refused(eng.set_random_sequences, 5, 10, SEED)
        assert refused(eng.calibrate, 5, 10, SEED, None, LAMBDA)
        assert eng.num_sequences == 4 and np.array_equal(eng.code_rows(2), rows)
        assert [bits(eng.profile_mu(p)) for p in range(len(KS))] == mu  # the queries answer, and nothing moved
    finally:
        eng.cost_hits_end()
    assert np.array_equal(eng.code_rows(2), rows)
    eng.set_random_sequences(5, 10, SEED)  # and accepted again once the batch has ended
    assert eng.num_sequences == 5


def test_bad_arguments_change_nothing(eng):
    eng.calibrate(8, LEN, SEED, FREQ, LAMBDA)
    mu = [bits(eng.profile_mu(p)) for p in range(len(KS))]
    eng.set_sequences(random_reads(99, 4, 30))
    rows = eng.code_rows(3)
    for lam in (0.0, -0.5, float("nan"), float("inf")):
        assert refused(eng.calibrate, 8, LEN, SEED, FREQ, lam)
    for nseq, length in ((0, LEN), (8, 0), (-1, LEN), (8, -1)):
        assert refused(eng.calibrate, nseq, length, SEED, FREQ, LAMBDA)
    for nseq, length in ((-1, LEN), (8, -1), (2**31 - 1, 2**31 - 2)):  # the last: code rows beyond 2^32
        assert refused(eng.set_random_sequences, nseq, length, SEED, FREQ)
    for freq in ([-1, 1, 1, 1], [float("nan"), 1, 1, 1], [0, 0, 0, 0]):
        assert refused(eng.calibrate, 8, LEN, SEED, freq, LAMBDA)
        assert refused(eng.set_random_sequences, 8, LEN, SEED, freq)
    assert eng.num_sequences == 4 and np.array_equal(eng.code_rows(3), rows)
    assert [bits(eng.profile_mu(p)) for p in range(len(KS))] == mu
    assert eng.calib_lambda == LAMBDA
    assert math.isnan(eng.profile_mu(-1)) and math.isnan(eng.profile_mu(len(KS)))


def test_seeds(eng):
    eng.calibrate(64, LEN, SEED, FREQ, LAMBDA)
    first = [bits(eng.profile_mu(p)) for p in range(len(KS))]
    rows = eng.code_rows(63)
    eng.calibrate(64, LEN, SEED, FREQ, LAMBDA)
    assert [bits(eng.profile_mu(p)) for p in range(len(KS))] == first
    assert np.array_equal(eng.code_rows(63), rows)
    eng.calibrate(64, LEN, SEED + 1, FREQ, LAMBDA)
    assert not np.array_equal(eng.code_rows(63), rows)
    assert [bits(eng.profile_mu(p)) for p in range(len(KS))] != first


def test_mu_is_nan_until_calibrated_and_after_what_changes_a_score():
    """on profiles from a HMMER3 file: dcp_hip_set_epsilon and _set_gencode work only on those"""
    import deciphon_amd

    with deciphon_amd.Engine(0) as e:
        assert math.isnan(e.profile_mu(0)) and math.isnan(e.calib_lambda)
        e.calibrate(8, LEN, SEED)  # no profiles: the sequences are set, and that is all
        assert e.num_sequences == 8 and math.isnan(e.calib_lambda)
        e.load_hmm(HMM, 1, 0.01)
        e.commit()
        n = e.num_profiles
        assert n >= 2 and all(math.isnan(e.profile_mu(p)) for p in range(n))
        assert refused(e.calibrate, 8, LEN, SEED, None, LAMBDA)  # no mode yet
        e.set_mode(True, False)

        def calibrated():
            e.calibrate(16, LEN, SEED, None, LAMBDA)
            mu = [e.profile_mu(p) for p in range(n)]
            assert all(np.isfinite(mu)) and e.calib_lambda == LAMBDA, mu
            return [bits(m) for m in mu]

        def gone():
            return all(math.isnan(e.profile_mu(p)) for p in range(n)) and math.isnan(e.calib_lambda)

        base = calibrated()
        e.set_epsilon(0.02)
        assert gone()
        assert calibrated() != base  # other tables, other scores
        e.set_epsilon(0.01)
        assert gone() and calibrated() == base
        e.set_gencode(11)
        assert gone() and calibrated()
        e.set_mode(False, False)
        assert gone() and calibrated() != base
        e.set_mode(True, False)
        e.set_gencode(1)
        assert calibrated() == base
        e.set_xtrans_table(np.zeros((0, 13), np.float32))
        assert gone() and calibrated() == base
        # profiles added later start at NaN; the others keep theirs
        e.load_hmm(HMM, 1, 0.01, 0, 1)
        e.commit()
        assert [bits(e.profile_mu(p)) for p in range(n)] == base and math.isnan(e.profile_mu(n))
        e.clear_profiles()
        assert math.isnan(e.profile_mu(0)) and math.isnan(e.calib_lambda)
