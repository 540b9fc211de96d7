"""CPU: the host side of calibration (include/deciphon_host.h): the pinned generator of the random reads against an
independent numpy restatement of its formula, the thresholds it draws bases by, and the Gumbel tail that turns a row's
lrt into an E-value."""
import ctypes
import math
import re

import numpy as np
import pytest

import deciphon_amd
from deciphon_amd import host
from deciphon_amd.hip import HipError

M64 = (1 << 64) - 1


def splitmix_u32(seed: int, idx) -> np.ndarray:
    """u of the formula, in numpy uint64 (which wraps mod 2^64), for an array of indices"""
    with np.errstate(over="ignore"):
        idx = np.asarray(idx, np.uint64)
        z = np.uint64(seed) + (idx + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return ((z ^ (z >> np.uint64(31))) >> np.uint64(32)).astype(np.uint64)


def bases_of(seed: int, first: int, n: int, t) -> np.ndarray:
    u = splitmix_u32(seed, np.arange(first, first + n, dtype=np.uint64))
    t = [np.uint64(int(v)) for v in t]
    return ((u >= t[0]).astype(np.uint8) + (u >= t[1]) + (u >= t[2])).astype(np.uint8)


def test_restatement_against_plain_integers():
    """the numpy restatement itself, against Python integers for a few indices"""
    for seed, idx in ((0, 0), (1, 7), (M64, 2**32 - 3), (12345, 2**40 + 1)):
        z = (seed + (idx + 1) * 0x9E3779B97F4A7C15) & M64
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        assert int(splitmix_u32(seed, [idx])[0]) == (z ^ (z >> 31)) >> 32


@pytest.mark.parametrize("first", [0, 2**32 - 3], ids=["idx0", "idx2^32-3"])
@pytest.mark.parametrize("seed", [0, 1, M64], ids=["seed0", "seed1", "seed2^64-1"])
def test_random_nt_is_the_formula(seed, first):
    for freq in (None, [0.1, 0.4, 0.3, 0.2]):
        t = host.random_thresholds(freq)
        got = host.random_nt(seed, 1000, first, freq)
        want = bases_of(seed, first, 1000, t)
        assert np.array_equal(got, want), (seed, first, freq)
    assert len(set(host.random_nt(seed, 1000, first).tolist())) == 4


def test_a_32_bit_index_would_show():
    """indices 2^32 apart draw other bases: the index is 64 bits wide"""
    assert not np.array_equal(host.random_nt(5, 1000, 0), host.random_nt(5, 1000, 2**32))


def test_thresholds():
    assert host.random_thresholds().tolist() == [2**30, 2**31, 3 * 2**30]
    assert host.random_thresholds([2, 2, 2, 2]).tolist() == [2**30, 2**31, 3 * 2**30]  # normalised by their sum
    draws = host.random_nt(3, 100000, 0, [1, 0, 1, 0])
    assert set(draws.tolist()) == {0, 2}
    assert abs(int((draws == 0).sum()) - 50000) < 1000  # five standard deviations are 790
    assert set(host.random_nt(3, 100000, 0, [0, 0, 0, 1]).tolist()) == {3}
    assert set(host.random_nt(3, 100000, 0, [0, 1, 0, 0]).tolist()) == {1}
    # t[j] = min(floor(cum_j 2^32), 2^32 - 1)
    assert host.random_thresholds([1, 0, 1, 0]).tolist() == [2**31, 2**31, 2**32 - 1]
    assert host.random_thresholds([0, 0, 0, 1]).tolist() == [0, 0, 0]


@pytest.mark.parametrize("freq", [[-1, 1, 1, 1], [float("nan"), 1, 1, 1], [0, 0, 0, 0], [1, 1, 1, -0.5],
                                  [float("inf"), 1, 1, 1]])
def test_bad_frequencies_are_refused(freq):
    with pytest.raises(HipError) as e:
        host.random_thresholds(freq)
    assert e.value.code == 8  # DCP_EFUNCUSE
    with pytest.raises(HipError):
        host.random_nt(0, 10, 0, freq)


def test_random_nt_refuses_bad_ranges():
    t = host.random_thresholds()
    lib = host._lib()
    out = np.zeros(4, np.uint8)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    assert lib.dcp_random_nt(0, p(t), -1, 4, p(out)) == 8
    assert lib.dcp_random_nt(0, p(t), 0, -1, p(out)) == 8
    assert lib.dcp_random_nt(0, None, 0, 4, p(out)) == 8
    assert lib.dcp_random_nt(0, p(t), 0, 4, None) == 8
    assert lib.dcp_random_nt(0, p(t), 0, 0, None) == 0


def evalue_ref(lrt, mu, lam, z):
    """the tail in double, from the fp32 values the C function is given"""
    lrt, mu, lam = float(np.float32(lrt)), float(np.float32(mu)), float(np.float32(lam))
    return z * (-math.expm1(-math.exp(-lam * (lrt - mu))))


@pytest.mark.parametrize("lrt,mu,lam,z", [(3.0, 1.0, 0.5, 10.0), (0.0, 7.25, 0.5, 1.0), (201.0, 1.0, 0.5, 1.0),
                                           (212.5, 12.5, 0.5, 1234.0), (35.7, -3.1, 0.5, 60.0), (1.0, 1.0, 0.6931472, 2.0),
                                           (-4.0, 9.0, 0.5, 3.0), (80.3, 11.9, 0.25, 1e6)])
def test_lrt_evalue(lrt, mu, lam, z):
    got, want = host.lrt_evalue(lrt, mu, lam, z), evalue_ref(lrt, mu, lam, z)
    assert want > 0 and abs(got - want) <= 1e-15 * want, (got, want)


def test_lrt_evalue_far_in_the_tail():
    """lrt - mu = 200 at lambda 0.5: exp(-100) = 3.7e-44, where the naive 1 - exp(-x) is 0"""
    x = math.exp(-0.5 * 200.0)
    assert 1.0 - math.exp(-x) == 0.0
    got = host.lrt_evalue(200.0, 0.0, 0.5, 1.0)
    assert got > 0 and abs(got - x) <= 1e-15 * x


def test_lrt_evalue_nan():
    assert math.isnan(host.lrt_evalue(3.0, float("nan"), 0.5, 10.0))
    assert math.isnan(host.lrt_evalue(float("nan"), 1.0, 0.5, 10.0))


NEW_SYMBOLS = ("dcp_random_thresholds", "dcp_random_nt", "dcp_lrt_evalue", "dcp_hip_set_random_sequences", "dcp_hip_calibrate",
               "dcp_hip_profile_mu", "dcp_hip_profile_calib_excluded", "dcp_hip_calib_lambda", "dcp_scan_calibrate",
               "dcp_scan_set_evalue", "dcp_scan_profile_mu")


def test_new_symbols_are_exported_and_declared():
    import os

    from dcp_testlib import ROOT

    lib = ctypes.CDLL(deciphon_amd.library_path())
    declared = "".join(open(os.path.join(ROOT, "include", h)).read() for h in ("deciphon.h", "deciphon_hip.h", "deciphon_host.h"))
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert re.search(r"\b%s\s*\(" % name, declared), name


def test_python_surface():
    from deciphon_amd.hip import Engine
    from deciphon_amd.scan import Scan

    for cls, names in ((Engine, ("set_random_sequences", "calibrate", "profile_mu")), (Scan, ("calibrate", "set_evalue", "profile_mu"))):
        for n in names:
            assert callable(getattr(cls, n)), (cls, n)
