"""Python mirror of python-core's `PressContext` (python-core/deciphon_core/press.py) over the C API of
include/deciphon.h, with ctypes instead of CFFI: HMMER3 text in, a pressed .dcp database out.  The emission tables
are computed on the GPU; without a gfx950 `open` raises DeciphonError (DCP_EFUNCUSE) and creates nothing."""
from __future__ import annotations

import ctypes as C
import os

from .hip import HipError as DeciphonError
from .hip import load_library

__all__ = ["Press", "DeciphonError"]

TIMING_KEYS = ("parse_model", "upload", "kernel", "copy_back", "wait", "write", "nodes", "bytes")


def _lib():
    L = load_library()
    if getattr(L, "_press_ready", False):
        return L
    vp, i32 = C.c_void_p, C.c_int
    L.dcp_press_new.restype = vp
    L.dcp_press_setup.argtypes = [vp, i32, C.c_float]
    L.dcp_press_open.argtypes = [vp, C.c_char_p, C.c_char_p]
    L.dcp_press_nproteins.argtypes = [vp]
    L.dcp_press_nproteins.restype = C.c_long
    L.dcp_press_next.argtypes = [vp]
    L.dcp_press_end.argtypes = [vp]
    L.dcp_press_end.restype = C.c_bool
    L.dcp_press_close.argtypes = [vp]
    L.dcp_press_del.argtypes = [vp]
    L.dcp_press_del.restype = None
    L.dcp_press_last_timing.argtypes = [vp, C.POINTER(C.c_double), i32]
    L._press_ready = True
    return L


class Press:
    """`with Press("x.hmm", "x.dcp", gencode=1, epsilon=0.01) as p: while not p.end(): p.next()`"""

    def __init__(self, hmm: str, db: str, gencode: int = 1, epsilon: float = 0.01):
        self._lib = _lib()
        self._hmm, self._db = os.fsencode(hmm), os.fsencode(db)
        self._cpress = self._lib.dcp_press_new()
        if not self._cpress:
            raise MemoryError()
        if rc := self._lib.dcp_press_setup(self._cpress, int(gencode), float(epsilon)):
            raise DeciphonError(rc)

    def open(self):
        if rc := self._lib.dcp_press_open(self._cpress, self._hmm, self._db):
            raise DeciphonError(rc)

    def close(self):
        if rc := self._lib.dcp_press_close(self._cpress):
            raise DeciphonError(rc)

    def end(self) -> bool:
        return bool(self._lib.dcp_press_end(self._cpress))

    def next(self):
        if rc := self._lib.dcp_press_next(self._cpress):
            raise DeciphonError(rc)

    def __enter__(self):
        self.open()
        return self

    def __exit__(self, *_):
        self.close()

    @property
    def nproteins(self) -> int:
        return int(self._lib.dcp_press_nproteins(self._cpress))

    def timing(self) -> dict:
        """dcp_press_last_timing: seconds per phase since open, nodes and bytes written."""
        out = (C.c_double * len(TIMING_KEYS))()
        self._lib.dcp_press_last_timing(self._cpress, out, len(TIMING_KEYS))
        return dict(zip(TIMING_KEYS, list(out)))

    def __del__(self):
        if getattr(self, "_cpress", None):
            self._lib.dcp_press_del(self._cpress)
            self._cpress = None
