"""Python mirror of python-core's wrapper classes over the C API of include/deciphon.h:
`Scan` (python-core/deciphon_core/scan.py:23-77), `Batch` (batch.py:9-30), `Sequence`
(sequence.py) and `DeciphonError` (error.py), over ctypes instead of CFFI."""
from __future__ import annotations

import ctypes as C
import dataclasses
import os

import numpy as np

from .hip import HipError as DeciphonError
from .hip import load_library, strands_code

__all__ = ["Scan", "Batch", "Sequence", "DeciphonError", "hit_on_read"]

_CALLBACK = C.CFUNCTYPE(None, C.c_void_p)


def _lib():
    L = load_library()
    if getattr(L, "_scan_ready", False):
        return L
    vp, i32 = C.c_void_p, C.c_int
    L.dcp_scan_new.restype = vp
    L.dcp_scan_del.argtypes = [vp]
    L.dcp_scan_del.restype = None
    L.dcp_scan_setup.argtypes = [vp, C.c_char_p, i32, i32, C.c_bool, C.c_bool, C.c_bool, _CALLBACK, vp]
    L.dcp_scan_setup_partition.argtypes = [vp, C.c_char_p, i32, i32, i32, C.c_bool, C.c_bool, _CALLBACK, vp]
    L.dcp_scan_setup_partition_balanced.argtypes = L.dcp_scan_setup_partition.argtypes
    L.dcp_scan_setup_hmm.argtypes = [vp, C.c_char_p, i32, C.c_float, C.c_bool, C.c_bool, _CALLBACK, vp]
    L.dcp_scan_set_epsilon.argtypes = [vp, C.c_float]
    L.dcp_scan_set_gencode.argtypes = [vp, i32]
    L.dcp_scan_calibrate.argtypes = [vp, i32, i32, C.c_uint64, vp, C.c_float]
    L.dcp_scan_set_evalue.argtypes = [vp, C.c_double, C.c_double]
    L.dcp_scan_profile_mu.argtypes = [vp, i32]
    L.dcp_scan_profile_mu.restype = C.c_float
    L.dcp_scan_calibrate_lengths.argtypes = [vp, i32, i32, vp, C.c_uint64, vp, C.c_float]
    L.dcp_scan_profile_mu_at.argtypes = [vp, i32, C.c_int64]
    L.dcp_scan_profile_mu_at.restype = C.c_double
    L.dcp_scan_profile_lambda.argtypes = [vp, i32]
    L.dcp_scan_profile_lambda.restype = C.c_float
    L.dcp_scan_set_strands.argtypes = [vp, i32]
    L.dcp_scan_strands.argtypes = [vp]
    L.dcp_scan_partition_range.argtypes = [vp, C.POINTER(i32), C.POINTER(i32)]
    L.dcp_scan_run.argtypes = [vp, vp, C.c_char_p]
    L.dcp_scan_interrupt.argtypes = [vp]
    L.dcp_scan_interrupt.restype = None
    L.dcp_scan_progress.argtypes = [vp]
    L.dcp_scan_num_products.argtypes = [vp]
    L.dcp_scan_num_products.restype = C.c_long
    L.dcp_scan_product.argtypes = [vp, C.c_long]
    L.dcp_scan_product.restype = C.c_char_p
    L.dcp_scan_last_timing.argtypes = [vp, C.POINTER(C.c_double), i32]
    L.dcp_scan_product_stats.argtypes = [vp, C.POINTER(C.c_int64), i32]
    L.dcp_batch_new.restype = vp
    L.dcp_batch_del.argtypes = [vp]
    L.dcp_batch_del.restype = None
    L.dcp_batch_add.argtypes = [vp, C.c_long, C.c_char_p, C.c_char_p]
    L.dcp_batch_reset.argtypes = [vp]
    L.dcp_batch_reset.restype = None
    L._scan_ready = True
    return L


def hit_on_read(row, read_length: int):
    """(start, stop, strand) of a product row's hit on the read AS GIVEN, 0-based and half-open.  `row`: a row of
    products.tsv, the string or its fields; a 12-column row (a scan of the plus strand) is a "+" row.  The row's own
    coordinates are on the scanned strand: a minus hit [ws + hs, ws + he) of the reverse complement of a read of L
    nucleotides lies at [L - (ws + he), L - (ws + hs)) of the read."""
    f = row.split("\t") if isinstance(row, str) else list(row)
    ws, hs, he = int(f[2]), int(f[5]), int(f[6])
    strand = f[12] if len(f) > 12 else "+"
    if strand == "+":
        return ws + hs, ws + he, "+"
    if strand != "-":
        raise ValueError(f"strand column {strand!r}")
    L = int(read_length)
    return L - (ws + he), L - (ws + hs), "-"


@dataclasses.dataclass
class Sequence:
    id: int
    name: str
    data: str


class Batch:
    def __init__(self):
        self._lib = _lib()
        self._cbatch = self._lib.dcp_batch_new()
        if not self._cbatch:
            raise MemoryError()

    def add(self, sequence: Sequence):
        if rc := self._lib.dcp_batch_add(self._cbatch, sequence.id, sequence.name.encode(), sequence.data.encode()):
            raise DeciphonError(rc)

    def reset(self):
        self._lib.dcp_batch_reset(self._cbatch)

    @property
    def cdata(self):
        return self._cbatch

    def __del__(self):
        if getattr(self, "_cbatch", None):
            self._lib.dcp_batch_del(self._cbatch)
            self._cbatch = None


class Scan:
    """Same constructor and methods as python-core's Scan.  `partition=(device, index, nparts)`
    (not in the reference) makes this scan own one contiguous profile partition on one GPU;
    `balanced=True` puts the partition boundaries where they balance the sum of core sizes.
    `strands="both"` (not in the reference either: dcp_scan_set_strands) scans the reverse complement of every read as
    well: products.tsv gains a 13th column `strand`, and a "-" row's coordinates and match column are on the reverse
    complement of the read as Batch.add keeps it (hit_on_read maps them back)."""

    def __init__(self, dbfile, port: int = 0, num_threads: int = 1, multi_hits: bool = True,
                 hmmer3_compat: bool = False, cache: bool = False, partition=None, on_window=None,
                 balanced: bool = False, progress_callback: bool = True, _hmm=None, strands="plus"):
        self._lib = _lib()
        strands = strands_code(strands)
        self._cscan = self._lib.dcp_scan_new()
        if not self._cscan:
            raise MemoryError()
        self.interrupted = False
        self._on_window = on_window

        def _cb(_userdata):
            if self._on_window is not None:
                try:
                    self._on_window()
                except BaseException:
                    self.interrupt()  # python-core/deciphon_core/scan.py:12-15
                    raise

        # python-core always hands the library a callback (an empty function: it lets Python raise KeyboardInterrupt
        # between windows); progress_callback=False hands it none, as a C caller may (c-core/test_scan.c:36-41)
        self._cb = _CALLBACK(_cb) if progress_callback else C.cast(None, _CALLBACK)
        path = os.fsencode(getattr(dbfile, "path", dbfile))
        if _hmm is not None:  # from_hmm: (gencode, epsilon)
            rc = self._lib.dcp_scan_setup_hmm(self._cscan, path, int(_hmm[0]), float(_hmm[1]), multi_hits,
                                              hmmer3_compat, self._cb, None)
        elif partition is None:
            rc = self._lib.dcp_scan_setup(self._cscan, path, port, num_threads, multi_hits, hmmer3_compat, cache,
                                          self._cb, None)
        else:
            device, index, nparts = partition
            setup = self._lib.dcp_scan_setup_partition_balanced if balanced else self._lib.dcp_scan_setup_partition
            rc = setup(self._cscan, path, device, index, nparts, multi_hits, hmmer3_compat, self._cb, None)
        if not rc:
            rc = self._lib.dcp_scan_set_strands(self._cscan, strands)
        if rc:
            self.free()
            raise DeciphonError(rc)

    @classmethod
    def from_hmm(cls, hmmfile, gencode: int = 1, epsilon: float = 0.01, multi_hits: bool = True,
                 hmmer3_compat: bool = False, on_window=None, progress_callback: bool = True, strands="plus"):
        """A scan straight from a HMMER3 text file (dcp_scan_setup_hmm, not in the reference): the tables are made
        on the GPU and stay there, no .dcp is written, and the rows are those of a scan of the file pressed at the
        same `gencode` and `epsilon`."""
        return cls(hmmfile, multi_hits=multi_hits, hmmer3_compat=hmmer3_compat, on_window=on_window,
                   progress_callback=progress_callback, _hmm=(gencode, epsilon), strands=strands)

    def set_strands(self, strands):
        """"plus" or "both" for every later run (dcp_scan_set_strands); allowed at any time between runs."""
        if rc := self._lib.dcp_scan_set_strands(self._cscan, strands_code(strands)):
            raise DeciphonError(rc)

    @property
    def strands(self) -> str:
        return "both" if self._lib.dcp_scan_strands(self._cscan) == 1 else "plus"

    def set_epsilon(self, epsilon: float):
        """A scan made by from_hmm at another error rate (dcp_scan_set_epsilon): the next run writes the rows of a
        fresh from_hmm at `epsilon`.  Not while run() is running."""
        if rc := self._lib.dcp_scan_set_epsilon(self._cscan, float(epsilon)):
            raise DeciphonError(rc)

    def set_gencode(self, gencode: int):
        """A scan made by from_hmm under another translation table (dcp_scan_set_gencode): the next run writes the
        rows of a fresh from_hmm at `gencode` and the error rate the scan is at.  Not while run() is running."""
        if rc := self._lib.dcp_scan_set_gencode(self._cscan, int(gencode)):
            raise DeciphonError(rc)

    def calibrate(self, nseq: int = 200, length: int = 300, seed: int = 42, freq=None, lam: float = 0.5):
        """Calibrates every profile on nseq random reads of `length` nucleotides, on the GPU (dcp_scan_calibrate): later
        runs print an E-value in the evalue column instead of nan.  lam = 0.5 is HMMER's conjectured ln 2 per bit, lrt
        being twice the log-odds in nats.  Wanted again after set_epsilon or set_gencode.  Not while run() is running."""
        f = None if freq is None else np.ascontiguousarray(freq, np.float32).reshape(4)
        ptr = None if f is None else f.ctypes.data_as(C.c_void_p)
        if rc := self._lib.dcp_scan_calibrate(self._cscan, int(nseq), int(length), int(seed) & (2**64 - 1), ptr, float(lam)):
            raise DeciphonError(rc)

    def calibrate_lengths(self, nseq: int = 200, lengths=(300, 1000, 3000, 10000), seed: int = 42, freq=None, lam: float = 0.5):
        """calibrate() at every length of the increasing ladder `lengths` (dcp_scan_calibrate_lengths): the E-value of a
        row then takes mu at the length of the row's window, linear in its logarithm between the rungs and beyond them
        (host.calib_mu_at).  lam = 0 fits one lambda per profile as well.  Not while run() is running."""
        f = None if freq is None else np.ascontiguousarray(freq, np.float32).reshape(4)
        ptr = None if f is None else f.ctypes.data_as(C.c_void_p)
        lens = np.ascontiguousarray(lengths, np.int32).reshape(-1)
        if rc := self._lib.dcp_scan_calibrate_lengths(self._cscan, int(nseq), len(lens), lens.ctypes.data_as(C.c_void_p),
                                                      int(seed) & (2**64 - 1), ptr, float(lam)):
            raise DeciphonError(rc)

    def profile_mu_at(self, i: int, length: int) -> float:
        """The Gumbel location of this scan's profile i at a window of `length` nucleotides; NaN when not calibrated."""
        return float(self._lib.dcp_scan_profile_mu_at(self._cscan, int(i), int(length)))

    def profile_lambda(self, i: int) -> np.float32:
        """lambda of this scan's profile i, passed or fitted; NaN when the scan is not calibrated."""
        return np.float32(self._lib.dcp_scan_profile_lambda(self._cscan, int(i)))

    def set_evalue(self, z: float = 0.0, max: float = float("inf")):
        """Z of the evalue column (<= 0: the sequences a run scans, reads x strands) and the limit of its rows: a
        calibrated run leaves out rows with E >= max (the reference's rule is max = 1).  dcp_scan_set_evalue."""
        if rc := self._lib.dcp_scan_set_evalue(self._cscan, float(z), float(max)):
            raise DeciphonError(rc)

    def profile_mu(self, i: int) -> np.float32:
        """The Gumbel location of this scan's profile i; NaN when the scan is not calibrated."""
        return np.float32(self._lib.dcp_scan_profile_mu(self._cscan, int(i)))

    def run(self, snap, batch: Batch):
        self.interrupted = False
        basedir = getattr(snap, "basedir", snap)
        if rc := self._lib.dcp_scan_run(self._cscan, batch.cdata, str(basedir).encode()):
            raise DeciphonError(rc)

    def partition_range(self):
        """(first profile, number of profiles) of the database this scan owns."""
        first, count = C.c_int(0), C.c_int(0)
        if rc := self._lib.dcp_scan_partition_range(self._cscan, C.byref(first), C.byref(count)):
            raise DeciphonError(rc)
        return first.value, count.value

    def products(self):
        n = self._lib.dcp_scan_num_products(self._cscan)
        return [self._lib.dcp_scan_product(self._cscan, i).decode() for i in range(n)]

    def last_timing(self) -> dict:
        """Where the wall time of the last run went (dcp_scan_last_timing): seconds per phase and counts."""
        keys = ("total_s", "reads_h2d_encode_s", "window_bookkeeping_s", "cost_pass_s", "path_pass_s", "rows_decode_s",
                "products_tsv_s", "rounds", "windows", "path_passes", "chunks", "largest_chunk_windows",
                "path_batches")
        buf = (C.c_double * len(keys))()
        n = self._lib.dcp_scan_last_timing(self._cscan, buf, len(keys))
        assert n == len(keys)
        return {k: (int(buf[i]) if i >= 7 else float(buf[i])) for i, k in enumerate(keys)}

    def product_stats(self) -> dict:
        """How the last run held its product rows (dcp_scan_product_stats): rows, run files written (0: every row
        stayed in memory), the most bytes of row text held at once, and the bytes of products.tsv."""
        keys = ("rows", "runs", "peak_bytes", "file_bytes")
        buf = (C.c_int64 * len(keys))()
        n = self._lib.dcp_scan_product_stats(self._cscan, buf, len(keys))
        assert n == len(keys)
        return {k: int(buf[i]) for i, k in enumerate(keys)}

    def interrupt(self):
        self.interrupted = True
        self._lib.dcp_scan_interrupt(self._cscan)

    def progress(self) -> int:
        return self._lib.dcp_scan_progress(self._cscan)

    def free(self):
        if getattr(self, "_cscan", None):
            self._lib.dcp_scan_del(self._cscan)
            self._cscan = None

    def __del__(self):
        self.free()

    def __enter__(self):
        return self

    def __exit__(self, *_):
        self.free()
