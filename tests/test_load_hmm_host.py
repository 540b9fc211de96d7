"""CPU: the HMMER3-file route (dcp_hip_load_hmm, dcp_scan_setup_hmm) as far as it goes without a GPU -- the symbols are
exported, and dcp_scan_setup_hmm tells its arguments apart, in the documented order, before it looks for a device; with
good arguments it is DCP_EFUNCUSE (there is no CPU fallback) and nothing is created next to the file."""
import ctypes as C
import os
import shutil

import pytest

import deciphon_amd
from dcp_testlib import GOLDEN

DCP_EFUNCUSE, DCP_EOPENHMM, DCP_EGENCODEID = 8, 22, 50
HMM = os.path.join(GOLDEN, "minifam.hmm")


def test_new_entry_points_are_exported():
    lib = C.CDLL(deciphon_amd.library_path())
    for name in ("dcp_hip_load_hmm", "dcp_hip_profile_floats", "dcp_hip_profile_read", "dcp_scan_setup_hmm"):
        assert hasattr(lib, name), name


@pytest.fixture
def cscan():
    from deciphon_amd.scan import _CALLBACK, _lib

    lib = _lib()
    x = lib.dcp_scan_new()
    assert x
    yield lambda path, gencode, eps: lib.dcp_scan_setup_hmm(x, os.fsencode(path), gencode, eps, True, False,
                                                           C.cast(None, _CALLBACK), None)
    lib.dcp_scan_del(x)


def test_setup_hmm_checks_its_arguments_before_the_device(cscan, tmp_path):
    hmm = str(tmp_path / "minifam.hmm")
    shutil.copy(HMM, hmm)
    missing = str(tmp_path / "missing.hmm")
    assert cscan(hmm, 7, 0.01) == DCP_EGENCODEID  # NCBI has no table 7
    assert cscan(missing, 7, 1.5) == DCP_EGENCODEID  # ... and it is checked first
    assert cscan(hmm, 1, 1.5) == DCP_EFUNCUSE
    assert cscan(hmm, 1, float("nan")) == DCP_EFUNCUSE
    assert cscan(missing, 1, 1.5) == DCP_EFUNCUSE  # epsilon before the file
    assert cscan(missing, 1, 0.01) == DCP_EOPENHMM
    if deciphon_amd.device_count() == 0:  # (with a device this is a scan set up: tests/test_gpu_load_hmm.py)
        assert cscan(hmm, 1, 0.01) == DCP_EFUNCUSE  # no CPU fallback
    assert sorted(os.listdir(tmp_path)) == ["minifam.hmm"]


def test_scan_from_hmm_raises_the_code(tmp_path):
    from deciphon_amd.scan import DeciphonError, Scan

    with pytest.raises(DeciphonError) as e:
        Scan.from_hmm(HMM, gencode=7)
    assert e.value.code == DCP_EGENCODEID
    with pytest.raises(DeciphonError) as e:
        Scan.from_hmm(str(tmp_path / "missing.hmm"))
    assert e.value.code == DCP_EOPENHMM
