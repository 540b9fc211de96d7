"""CPU: the host side of the calibration over a ladder of read lengths.  dcp_calib_mu_at (include/deciphon_host.h), the
one statement of mu at a window length, against a float64 numpy statement of the same rule; the float64 solver the GPU
test holds the fit kernel to (tests/calib_ladder.py), against known parameters and against a Newton solver of the same
equation; and the new symbols."""
import ctypes
import math
import re

import numpy as np
import pytest

import calib_ladder
import deciphon_amd
from deciphon_amd import host

LENS = (300, 1000, 3000, 10000)
MU = (-23.25, -25.5, -27.75, -30.875)


def mu_at_ref(lens, mu, length):
    """the rule in float64: the line through the two usable rungs around `length` in ln length, the end segment's beyond
    the ends"""
    mu = np.asarray(mu, np.float32).astype(np.float64)
    use = [j for j in range(len(lens)) if not np.isnan(mu[j])]
    if not use:
        return math.nan
    for j in use:
        if lens[j] == length:
            return float(mu[j])
    if len(use) == 1:
        return float(mu[use[0]])
    above = [k for k, j in enumerate(use) if lens[j] > length]
    k = min(max(above[0] if above else len(use) - 1, 1), len(use) - 1)
    a, b = use[k - 1], use[k]
    t = np.log(np.float64(length) / np.float64(lens[a])) / np.log(np.float64(lens[b]) / np.float64(lens[a]))
    return float(mu[a] + (mu[b] - mu[a]) * t)


def close(got, want, mu):
    tol = 1e-14 * max(1.0, float(np.nanmax(np.abs(np.asarray(mu, np.float64)))))
    assert abs(got - want) <= tol, (got, want, tol)


def test_exact_at_the_rungs():
    for j, length in enumerate(LENS):
        assert host.calib_mu_at(LENS, MU, length) == float(np.float32(MU[j]))
    odd = [np.float32(-23.3), np.float32(-27.7)]  # no exact double behind them but their own
    assert host.calib_mu_at((300, 3000), odd, 300) == float(odd[0])
    assert host.calib_mu_at((300, 3000), odd, 3000) == float(odd[1])


@pytest.mark.parametrize("length", [301, 550, 999, 1001, 1800, 2999, 5500, 9999])
def test_between_the_rungs(length):
    got = host.calib_mu_at(LENS, MU, length)
    close(got, mu_at_ref(LENS, MU, length), MU)
    j = max(k for k in range(4) if LENS[k] < length)
    assert MU[j + 1] < got < MU[j]


@pytest.mark.parametrize("length", [1, 7, 299, 10001, 100000, 2**40])
def test_the_end_segments_continue(length):
    got = host.calib_mu_at(LENS, MU, length)
    close(got, mu_at_ref(LENS, MU, length), MU)
    assert got > MU[0] if length < LENS[0] else got < MU[-1]  # not clamped
    # the statement, spelled out once more for the two ends
    a, b = (0, 1) if length < LENS[0] else (2, 3)
    slope = (MU[b] - MU[a]) / math.log(LENS[b] / LENS[a])
    assert abs(got - (MU[a] + slope * math.log(length / LENS[a]))) <= 1e-12 * abs(got)


def test_one_rung_is_a_constant():
    for length in (1, 299, 300, 301, 10**6):
        assert host.calib_mu_at([300], [-23.25], length) == -23.25


NAN = float("nan")


@pytest.mark.parametrize("mu", [(-23.25, NAN, -27.75, -30.875), (NAN, -25.5, -27.75, -30.875), (-23.25, -25.5, -27.75, NAN),
                                (NAN, NAN, -27.75, -30.875), (-23.25, NAN, NAN, NAN), (NAN, NAN, -27.75, NAN)],
                         ids=["middle", "first", "last", "first-two", "all-but-first", "all-but-one"])
def test_nan_rungs_are_skipped(mu):
    for length in (7, 300, 550, 1000, 1800, 3000, 5500, 10000, 50000):
        got, want = host.calib_mu_at(LENS, mu, length), mu_at_ref(LENS, mu, length)
        assert not math.isnan(want)
        close(got, want, mu)
    for j, length in enumerate(LENS):
        if not math.isnan(mu[j]):
            assert host.calib_mu_at(LENS, mu, length) == mu[j]
    if sum(not math.isnan(m) for m in mu) == 1:
        only = [m for m in mu if not math.isnan(m)][0]
        assert all(host.calib_mu_at(LENS, mu, length) == only for length in (1, 550, 99999))


def test_a_skipped_rung_is_bridged():
    """at the length of a NaN rung the line of its neighbours holds"""
    got = host.calib_mu_at(LENS, (-23.25, NAN, -27.75, -30.875), 1000)
    want = -23.25 + (-27.75 + 23.25) * math.log(1000 / 300) / math.log(3000 / 300)
    assert abs(got - want) <= 1e-13


def test_bad_arguments_give_nan():
    assert math.isnan(host.calib_mu_at(LENS, (NAN,) * 4, 300))
    assert math.isnan(host.calib_mu_at(LENS, MU, 0))
    assert math.isnan(host.calib_mu_at(LENS, MU, -5))
    assert math.isnan(host.calib_mu_at([], [], 300))
    assert math.isnan(host.calib_mu_at((300, 300), (-1.0, -2.0), 300))
    assert math.isnan(host.calib_mu_at((300, 200), (-1.0, -2.0), 300))
    assert math.isnan(host.calib_mu_at((0, 200), (-1.0, -2.0), 300))
    lib = host._lib()
    lens, mu = np.array(LENS, np.int32), np.array(MU, np.float32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    assert math.isnan(lib.dcp_calib_mu_at(4, None, p(mu), 300))
    assert math.isnan(lib.dcp_calib_mu_at(4, p(lens), None, 300))
    assert math.isnan(lib.dcp_calib_mu_at(0, p(lens), p(mu), 300))
    assert lib.dcp_calib_mu_at(4, p(lens), p(mu), 300) == MU[0]


# ---- the yardstick of the GPU test -----------------------------------------------------------------------------

def newton_lambda(rungs):
    """the same equation by Newton's method from the moment estimate, in float64"""
    ys = calib_ladder.informative([calib_ladder.kept_of(x) for x in rungs])
    ss = sum(((y - y.mean()) ** 2).sum() for y in ys)
    lam = math.pi / math.sqrt(6.0 * ss / sum(len(y) - 1 for y in ys))
    for _ in range(100):
        g = dg = 0.0
        for y in ys:
            e = np.exp(-lam * y)
            r = (y * e).sum() / e.sum()
            g += len(y) * (1.0 / lam - y.mean() + r)
            dg += len(y) * (-1.0 / lam**2 - (y * y * e).sum() / e.sum() + r * r)
        step = g / dg
        while lam - step <= 0:
            step /= 2
        lam -= step
        if abs(step) <= 1e-15 * lam:
            break
    return lam


def test_the_solver_finds_known_parameters():
    rng = np.random.default_rng(20261)
    true_mu = [-25.0 - 1.5 * j for j in range(3)]
    scores = [rng.gumbel(m, 1.0 / 0.5, 20000) for m in true_mu]
    lam, mu = calib_ladder.fit(scores)
    print("lambda", lam, "mu", mu)
    assert abs(lam - 0.5) <= 0.05 * 0.5
    for got, want in zip(mu, true_mu):
        assert abs(got - want) <= 0.1
    # at the fixed lambda the locations are the closed form's
    _, fixed = calib_ladder.fit(scores, 0.5)
    for got, want in zip(fixed, true_mu):
        assert abs(got - want) <= 0.1


@pytest.mark.parametrize("sizes", [(2,), (3,), (64,), (200,), (2, 3, 64, 200)], ids=str)
def test_bisection_and_newton_agree(sizes):
    rng = np.random.default_rng(sum(sizes))
    scores = [rng.gumbel(-25.0 - j, 2.0, n).astype(np.float32) for j, n in enumerate(sizes)]
    a, b = calib_ladder.solve_lambda([calib_ladder.kept_of(x) for x in scores]), newton_lambda(scores)
    print(sizes, a, b, abs(a - b) / b)
    assert a > 0 and abs(a - b) <= 1e-12 * b


def test_the_solver_leaves_out_what_the_kernel_leaves_out():
    x = np.array([-20.0, -22.5, -19.0, -24.0], np.float32)
    lam, mu = calib_ladder.fit([x, np.array([np.inf, np.nan], np.float32), np.array([-21.0, np.inf], np.float32),
                                np.array([-20.0, -20.0], np.float32)])
    alone, mu_alone = calib_ladder.fit([x])
    assert lam == alone and mu[0] == mu_alone[0]  # the other rungs carry no scale
    assert math.isnan(mu[1]) and mu[2] == -21.0 and mu[3] == -20.0
    lam, mu = calib_ladder.fit([np.array([-20.0, -20.0]), np.array([-21.0])])
    assert math.isnan(lam) and all(math.isnan(m) for m in mu)


# ---- the surface -----------------------------------------------------------------------------------------------

NEW_SYMBOLS = ("dcp_calib_mu_at", "dcp_hip_calibrate_lengths", "dcp_hip_calib_num_lengths", "dcp_hip_calib_length",
               "dcp_hip_profile_mu_rung", "dcp_hip_profile_calib_excluded_rung", "dcp_hip_profile_lambda", "dcp_hip_profile_mu_at",
               "dcp_scan_calibrate_lengths", "dcp_scan_profile_mu_at", "dcp_scan_profile_lambda")


def test_new_symbols_are_exported_and_declared():
    import os

    from dcp_testlib import ROOT

    lib = ctypes.CDLL(deciphon_amd.library_path())
    declared = "".join(open(os.path.join(ROOT, "include", h)).read() for h in ("deciphon.h", "deciphon_hip.h", "deciphon_host.h"))
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert re.search(r"\b%s\s*\(" % name, declared), name
    assert re.search(r"#define\s+DCP_CALIB_MAX_LENS\s+16\b", declared)


def test_python_surface():
    from deciphon_amd.hip import Engine
    from deciphon_amd.scan import Scan

    for cls, names in ((Engine, ("calibrate_lengths", "profile_mu_rung", "profile_calib_excluded_rung", "profile_lambda", "profile_mu_at")),
                       (Scan, ("calibrate_lengths", "profile_mu_at", "profile_lambda"))):
        for n in names:
            assert callable(getattr(cls, n)), (cls, n)
    assert isinstance(Engine.calib_lengths, property)
    assert callable(host.calib_mu_at)


def test_null_engine_is_refused():
    lib = ctypes.CDLL(deciphon_amd.library_path())
    lib.dcp_hip_calibrate_lengths.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64,
                                              ctypes.c_void_p, ctypes.c_float]
    lens = np.array([30, 60], np.int32)
    assert lib.dcp_hip_calibrate_lengths(None, 8, 2, lens.ctypes.data_as(ctypes.c_void_p), 1, None, 0.5) == 8  # DCP_EFUNCUSE
    lib.dcp_hip_profile_mu_at.restype = ctypes.c_double
    lib.dcp_hip_profile_mu_at.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int64]
    assert math.isnan(lib.dcp_hip_profile_mu_at(None, 0, 300))
    assert lib.dcp_hip_calib_num_lengths(None) == 0
