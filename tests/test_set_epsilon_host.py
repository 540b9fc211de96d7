"""CPU: what dcp_hip_set_epsilon and dcp_scan_set_epsilon do without a GPU -- the list of workgroups of the
re-emission kernel (dcp_reemit_tiles, include/deciphon_host.h) and the argument checks that come before the device."""
import ctypes as C
import math

import numpy as np
import pytest

from deciphon_amd import host

DCP_EFUNCUSE = 8


def expected(Kp):
    return [(i, k) for i, kp in enumerate(Kp) for k in range(0, int(kp), 64)]


def random_Kp():
    rng = np.random.default_rng(17)
    return (64 * rng.integers(1, 40, size=200)).tolist()


@pytest.mark.parametrize("Kp", [[64], [128], [16384], [64, 128, 16384], [16384, 64, 64, 128], random_Kp()],
                         ids=["64", "128", "16384", "mixed", "long-first", "random-200"])
def test_reemit_tiles_lists_every_tile_once_in_profile_order(Kp):
    want = expected(Kp)
    assert len(want) == sum(Kp) // 64
    count, profile, k0 = host.reemit_tiles(Kp, len(want) + 5)
    assert count == len(want)
    assert list(zip(profile[:count].tolist(), k0[:count].tolist())) == want
    assert (profile[count:] == -1).all() and (k0[count:] == -1).all()  # nothing beyond the count


@pytest.mark.parametrize("cap", [0, 1, 7])
def test_reemit_tiles_with_a_cap_below_the_count(cap):
    Kp = [64, 128, 16384] + random_Kp()
    want = expected(Kp)
    count, profile, k0 = host.reemit_tiles(Kp, len(want))
    assert count == len(want)
    # the same call into arrays with room, told that they hold `cap`: the count is the whole one, and nothing is
    # written beyond `cap`
    L = host._lib()
    p = np.full(len(want), -1, np.int32)
    k = np.full(len(want), -1, np.int32)
    a = np.ascontiguousarray(Kp, np.int32)
    got = L.dcp_reemit_tiles(len(a), a.ctypes.data_as(C.c_void_p), p.ctypes.data_as(C.c_void_p),
                             k.ctypes.data_as(C.c_void_p), cap)
    assert got == len(want)
    assert list(zip(p[:cap].tolist(), k[:cap].tolist())) == want[:cap]
    assert (p[cap:] == -1).all() and (k[cap:] == -1).all()
    if cap == 0:  # the arrays may then be NULL
        assert L.dcp_reemit_tiles(len(a), a.ctypes.data_as(C.c_void_p), None, None, 0) == len(want)


def test_reemit_tiles_of_no_profiles():
    assert host.reemit_tiles([], 4)[0] == 0


def test_engine_calls_check_their_arguments_without_a_gpu():
    from deciphon_amd import hip

    L = hip.load_library()
    assert L.dcp_hip_set_epsilon(None, 0.01) == DCP_EFUNCUSE
    assert math.isnan(L.dcp_hip_profile_epsilon(None, 0))
    assert L.dcp_hip_dist_bytes(None) == 0


def test_scan_set_epsilon_on_a_scan_not_set_up(capfd):
    from deciphon_amd import scan

    L = scan._lib()
    assert L.dcp_scan_set_epsilon(None, 0.01) == DCP_EFUNCUSE
    s = L.dcp_scan_new()
    assert s
    try:
        assert L.dcp_scan_set_epsilon(s, 0.01) == DCP_EFUNCUSE
        assert L.dcp_scan_set_epsilon(s, 2.0) == DCP_EFUNCUSE
    finally:
        L.dcp_scan_del(s)
    capfd.readouterr()
