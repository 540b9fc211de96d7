"""ctypes binding of include/deciphon_host.h: the .dcp reader and the scalar
bookkeeping of process_window (windows, trellis_unzip, hit spans).  No GPU needed."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from .hip import HipError, load_library

TABLE_SIZE = 1364


class _Window(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("core_size", "seq_size", "start", "stop", "idx", "last_hit_pos")]


def _lib():
    L = load_library()
    if getattr(L, "_host_ready", False):
        return L
    vp, i32 = C.c_void_p, C.c_int
    L.dcp_db_open.argtypes = [C.c_char_p, C.POINTER(vp)]
    L.dcp_db_close.argtypes = [vp]
    L.dcp_db_close.restype = None
    L.dcp_db_num_proteins.argtypes = [vp]
    L.dcp_db_epsilon.argtypes = [vp]
    L.dcp_db_epsilon.restype = C.c_float
    L.dcp_db_entry_dist.argtypes = [vp]
    L.dcp_db_has_ga.argtypes = [vp]
    L.dcp_db_protein_offset.argtypes = [vp, i32]
    L.dcp_db_protein_offset.restype = C.c_int64
    L.dcp_db_protein_core_size.argtypes = [vp, i32, C.POINTER(i32)]
    L.dcp_db_read_protein.argtypes = [vp, i32, vp, vp, vp, vp, vp, C.c_char_p, C.c_char_p]
    L.dcp_db_read_nuclt_dist.argtypes = [vp, i32, vp, vp, C.POINTER(i32)]
    L.dcp_decode_quasi_codon.argtypes = [C.c_float, vp, vp, vp, i32, vp]
    L.dcp_gencode_amino_of.argtypes = [i32, vp]
    L.dcp_gencode_amino_of.restype = C.c_char
    L.dcp_db_core_sizes.argtypes = [vp, vp]
    L.dcp_db_partition_bounds.argtypes = [vp, i32, i32, vp]
    L.dcp_partition_bounds_of.argtypes = [i32, vp, i32, i32, vp]
    L.dcp_partition_size.argtypes = [C.c_long, C.c_long, C.c_long]
    L.dcp_partition_size.restype = C.c_long
    L.dcp_window_count.argtypes = [C.c_int64, i32]
    L.dcp_window_count.restype = C.c_int64
    L.dcp_code_rows_of.argtypes = [vp, C.c_int64, i32, vp]
    L.dcp_cost_order_map.argtypes = [i32, i32, vp]
    L.dcp_row_lane_offsets.argtypes = [i32, i32, i32, i32, vp]
    L.dcp_reemit_tiles.argtypes = [i32, vp, vp, vp, C.c_int64]
    L.dcp_reemit_tiles.restype = C.c_int64
    L.dcp_scan_plan_chunks.argtypes = [i32, vp, i32, vp, C.c_double, C.c_double, C.c_int64, C.c_int64, i32, vp, vp,
                                       C.POINTER(i32)]
    L.dcp_path_plan_of.argtypes = [i32, i32, vp, vp, vp, vp, vp, i32, C.c_int64, i32, C.c_int64, i32, vp, vp, vp, vp, vp, vp,
                                   C.POINTER(i32), C.POINTER(i32)]
    L.dcp_stage_plan_of.argtypes = [i32, vp, i32, vp, i32, vp, vp, i32, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                    C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_char_p)]
    L.dcp_cost_schedule_of.argtypes = [vp, vp, vp, vp, vp, i32, i32, vp]
    L.dcp_trellis_arena_of.argtypes = [i32, vp, vp, vp]
    L.dcp_trellis_arena_of.restype = C.c_int64
    L.dcp_engine_core_size.argtypes = [i32, vp]
    L.dcp_engine_pack_shape.argtypes = [i32, vp]
    L.dcp_scan_walk_new.argtypes = [i32, vp, i32, vp]
    L.dcp_scan_walk_new.restype = vp
    L.dcp_scan_walk_del.argtypes = [vp]
    L.dcp_scan_walk_del.restype = None
    L.dcp_scan_walk_chunk_windows.argtypes = [vp, vp, C.c_int64, vp, vp]
    L.dcp_scan_walk_chunk_scored.argtypes = [vp, vp, vp, i32, vp, vp]
    L.dcp_scan_walk_all_pairs.argtypes = [vp]
    L.dcp_scan_walk_waiting.argtypes = [vp, i32]
    L.dcp_scan_walk_take.argtypes = [vp, i32, C.POINTER(vp)]
    L.dcp_scan_walk_cost_scored.argtypes = [vp, i32, vp, vp]
    L.dcp_scan_walk_path_walked.argtypes = [vp, vp, vp, C.POINTER(vp)]
    L.dcp_scan_walk_windows.argtypes = [vp]
    L.dcp_scan_walk_take_queued.argtypes = [vp]
    for f in ("waiting", "take", "path_walked", "windows", "take_queued"):
        getattr(L, "dcp_scan_walk_" + f).restype = C.c_int64
    L.dcp_product_runs_new.argtypes = [C.c_char_p, C.c_int64]
    L.dcp_product_runs_new.restype = vp
    L.dcp_product_runs_del.argtypes = [vp]
    L.dcp_product_runs_del.restype = None
    L.dcp_product_runs_add.argtypes = [vp, i32, vp, vp, vp, vp]
    L.dcp_product_runs_close.argtypes = [vp, C.c_char_p]
    L.dcp_product_runs_num_rows.argtypes = [vp]
    L.dcp_product_runs_num_rows.restype = C.c_long
    L.dcp_product_runs_row.argtypes = [vp, C.c_long]
    L.dcp_product_runs_row.restype = C.c_char_p
    L.dcp_product_runs_stats.argtypes = [vp, vp]
    L.dcp_window_setup.argtypes = [C.POINTER(_Window), i32, i32]
    L.dcp_window_setup.restype = None
    L.dcp_window_next.argtypes = [C.POINTER(_Window)]
    L.dcp_trellis_unzip.argtypes = [i32, i32, vp, vp, i32, vp, vp, C.POINTER(i32)]
    L.dcp_path_hit.argtypes = [i32, vp, vp, vp]
    L.dcp_state_name_of.argtypes = [i32, C.c_char_p]
    L.dcp_state_name_of.restype = None
    L.dcp_state_is_mute_id.argtypes = [i32]
    L.dcp_lrt_of.argtypes = [C.c_float, C.c_float]
    L.dcp_lrt_of.restype = C.c_float
    L.dcp_random_thresholds.argtypes = [vp, vp]
    L.dcp_random_nt.argtypes = [C.c_uint64, vp, C.c_int64, C.c_int64, vp]
    L.dcp_lrt_evalue.argtypes = [C.c_float, C.c_float, C.c_float, C.c_double]
    L.dcp_lrt_evalue.restype = C.c_double
    L.dcp_calib_mu_at.argtypes = [i32, vp, vp, C.c_int64]
    L.dcp_calib_mu_at.restype = C.c_double
    L.dcp_hmm_open.argtypes = [C.c_char_p, i32, C.POINTER(vp)]
    L.dcp_hmm_close.argtypes = [vp]
    L.dcp_hmm_close.restype = None
    L.dcp_hmm_count.argtypes = [vp]
    L.dcp_hmm_count.restype = C.c_long
    L.dcp_hmm_next.argtypes = [vp]
    L.dcp_hmm_end.argtypes = [vp]
    L.dcp_hmm_core_size.argtypes = [vp]
    L.dcp_hmm_has_ga.argtypes = [vp]
    L.dcp_hmm_read.argtypes = [vp, vp, vp, vp, vp, C.c_char_p, C.c_char_p]
    L.dcp_hmm_read_lodds.argtypes = [vp, vp]
    L.dcp_hmm_models.argtypes = [i32, vp, vp]
    L.dcp_regencode_entries.argtypes = [i32, C.c_int64, vp, i32, vp]
    L._host_ready = True
    return L


class HmmFile:
    """A HMMER3 text file read as press reads it (include/deciphon_host.h dcp_hmm_*): iterating yields one dict per
    profile with accession, consensus, core_size, has_ga, trans[(K+1), 7], BMk[K], and nucltp[(K+3), 4] /
    codonm[(K+3), 125] (0 = null, 1 = background, 2 + n = node n) -- the fields press writes, emission tables
    aside.  Host code only: no GPU is needed."""

    def __init__(self, path: str, gencode: int = 1):
        self.lib = _lib()
        h = C.c_void_p()
        rc = self.lib.dcp_hmm_open(os.fsencode(path), int(gencode), C.byref(h))
        if rc:
            raise HipError(rc, path)
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.lib.dcp_hmm_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *_):
        self.close()

    def __len__(self):
        """press.c count_proteins: the HMMER3/f lines of the file."""
        return int(self.lib.dcp_hmm_count(self.h))

    def next(self):
        """The next profile, or None at the end of the file; raises HipError on a malformed profile."""
        if rc := self.lib.dcp_hmm_next(self.h):
            raise HipError(rc)
        if self.lib.dcp_hmm_end(self.h):
            return None
        K = self.lib.dcp_hmm_core_size(self.h)
        trans = np.zeros((K + 1, 7), np.float32)
        BMk = np.zeros(K, np.float32)
        nucltp = np.zeros((K + 3, 4), np.float32)
        codonm = np.zeros((K + 3, 125), np.float32)
        acc = C.create_string_buffer(32)
        cons = C.create_string_buffer(K + 1)
        p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        if rc := self.lib.dcp_hmm_read(self.h, p(trans), p(BMk), p(nucltp), p(codonm), acc, cons):
            raise HipError(rc)
        lodds = np.zeros((K, 20), np.float32)
        if rc := self.lib.dcp_hmm_read_lodds(self.h, p(lodds)):
            raise HipError(rc)
        return dict(accession=acc.value.decode(), consensus=cons.value.decode(), core_size=K,
                    has_ga=bool(self.lib.dcp_hmm_has_ga(self.h)), trans=trans, BMk=BMk, nucltp=nucltp, codonm=codonm,
                    lodds=lodds)

    def __iter__(self):
        while (p := self.next()) is not None:
            yield p

    @staticmethod
    def models(gencode: int = 1):
        """(nucltp[2, 4], codonm[2, 125]): the null model, then the background, under translation table `gencode` --
        entries 0 and 1 of every profile of a file opened under it (dcp_hmm_models); no file is needed."""
        return hmm_models(gencode)


ENTRY_FLOATS = 132  # one kept entry (csrc/press_kernel.h): nucltp[4], codonm[125], 3 floats of padding


def hmm_models(gencode: int = 1):
    """See HmmFile.models."""
    nucltp = np.zeros((2, 4), np.float32)
    codonm = np.zeros((2, 125), np.float32)
    if rc := _lib().dcp_hmm_models(int(gencode), nucltp.ctypes.data_as(C.c_void_p), codonm.ctypes.data_as(C.c_void_p)):
        raise HipError(rc)
    return nucltp, codonm


def regencode_entries(gencode: int, lodds, max_threads: int = 16) -> np.ndarray:
    """entries float32[n, 132] -- nucltp[4], codonm[125], padding -- of n nodes under translation table `gencode`,
    from their amino log-odds lodds[n, 20] (a profile's "lodds" of HmmFile, which hold under every table): what
    Engine.set_gencode puts in place of the kept distributions (dcp_regencode_entries)."""
    lo = np.ascontiguousarray(lodds, np.float32).reshape(-1, 20)
    out = np.full((len(lo), ENTRY_FLOATS), np.nan, np.float32)
    if rc := _lib().dcp_regencode_entries(int(gencode), len(lo), lo.ctypes.data_as(C.c_void_p), int(max_threads),
                                          out.ctypes.data_as(C.c_void_p)):
        raise HipError(rc)
    return out


class Database:
    """A pressed .dcp file (replaces database_reader + protein_reader + protein_unpack)."""

    def __init__(self, path: str):
        self.lib = _lib()
        h = C.c_void_p()
        rc = self.lib.dcp_db_open(os.fsencode(path), C.byref(h))
        if rc:
            raise HipError(rc, path)
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.lib.dcp_db_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        return self.lib.dcp_db_num_proteins(self.h)

    @property
    def epsilon(self) -> float:
        return float(self.lib.dcp_db_epsilon(self.h))

    @property
    def entry_dist(self) -> int:
        return self.lib.dcp_db_entry_dist(self.h)

    @property
    def has_ga(self) -> bool:
        return bool(self.lib.dcp_db_has_ga(self.h))

    def offset(self, i: int) -> int:
        return int(self.lib.dcp_db_protein_offset(self.h, i))

    def core_sizes(self) -> np.ndarray:
        K = np.zeros(len(self), np.int32)
        if rc := self.lib.dcp_db_core_sizes(self.h, K.ctypes.data_as(C.c_void_p)):
            raise HipError(rc)
        return K

    def partition_bounds(self, nparts: int, balanced: bool = False) -> np.ndarray:
        """first[nparts + 1]: partition p = proteins first[p] .. first[p+1]-1 (c-core/protein_reader.c:112-128,
        or boundaries that balance the sum of core sizes)."""
        first = np.zeros(nparts + 1, np.int32)
        if rc := self.lib.dcp_db_partition_bounds(self.h, nparts, int(balanced), first.ctypes.data_as(C.c_void_p)):
            raise HipError(rc)
        return first

    def protein(self, i: int) -> dict:
        k = C.c_int(0)
        rc = self.lib.dcp_db_protein_core_size(self.h, i, C.byref(k))
        if rc:
            raise HipError(rc)
        K = k.value
        trans = np.zeros((K + 1, 7), np.float32)
        emission = np.zeros((K + 1, TABLE_SIZE), np.float32)
        BMk = np.zeros(K, np.float32)
        null = np.zeros(TABLE_SIZE, np.float32)
        bg = np.zeros(TABLE_SIZE, np.float32)
        acc = C.create_string_buffer(32)
        cons = C.create_string_buffer(K + 1)
        p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        rc = self.lib.dcp_db_read_protein(self.h, i, p(trans), p(emission), p(BMk), p(null), p(bg), acc, cons)
        if rc:
            raise HipError(rc)
        nucltp = np.zeros((K + 3, 4), np.float32)
        codonm = np.zeros((K + 3, 125), np.float32)
        gencode = C.c_int(0)
        rc = self.lib.dcp_db_read_nuclt_dist(self.h, i, p(nucltp), p(codonm), C.byref(gencode))
        if rc:
            raise HipError(rc)
        # nucltp / codonm: entry 0 = null model, 1 = background, 2 + n = node n (what decoder_setup takes)
        return dict(core_size=K, accession=acc.value.decode(), consensus=cons.value.decode(), trans=trans,
                    emission=emission, BMk=BMk, null_emission=null, bg_emission=bg, gencode=gencode.value,
                    nucltp=nucltp, codonm=codonm)


def partition_bounds(core_sizes, nparts: int, balanced: bool = False) -> np.ndarray:
    """first[nparts + 1] for profiles of the given core sizes (see Database.partition_bounds)."""
    K = np.ascontiguousarray(core_sizes, np.int32)
    first = np.zeros(nparts + 1, np.int32)
    if rc := _lib().dcp_partition_bounds_of(len(K), K.ctypes.data_as(C.c_void_p), nparts, int(balanced),
                                            first.ctypes.data_as(C.c_void_p)):
        raise HipError(rc)
    return first


def partition_size(nelems: int, nparts: int, idx: int) -> int:
    return int(_lib().dcp_partition_size(nelems, nparts, idx))


class WindowIter:
    """window_setup / window_next / window_set_last_hit_position (c-core/window.c)."""

    def __init__(self, seq_size: int, core_size: int):
        self.lib = _lib()
        self.w = _Window()
        self.lib.dcp_window_setup(C.byref(self.w), seq_size, core_size)

    def next(self):
        if not self.lib.dcp_window_next(C.byref(self.w)):
            return None
        return self.w.idx, self.w.start, self.w.stop

    def set_last_hit_position(self, pos: int) -> None:
        self.w.last_hit_pos = pos


def code_rows_of(nt, minus: bool = False) -> np.ndarray:
    """The code rows of one read of nucleotide indices 0..3 as the engine holds them, uint32 [len + 1][8]
    (dcp_code_rows_of): of the read as given, or -- minus -- of its reverse complement 3 - nt[::-1]."""
    nt = np.ascontiguousarray(nt, np.uint8)
    rows = np.empty((len(nt) + 1, 8), np.uint32)
    rc = _lib().dcp_code_rows_of(nt.ctypes.data_as(C.c_void_p), len(nt), int(bool(minus)), rows.ctypes.data_as(C.c_void_p))
    if rc:
        raise HipError(rc)
    return rows


def window_count(seq_size: int, core_size: int) -> int:
    """Windows of the no-hit chain of one (read, profile) pair (what WindowIter walks when nothing hits)."""
    return int(_lib().dcp_window_count(int(seq_size), int(core_size)))


def reemit_tiles(Kp, cap: int):
    """(count, profile int32[cap], k0 int32[cap]): the (profile, k0) workgroup list of Engine.set_epsilon's kernel for
    profiles of padded lengths Kp (dcp_reemit_tiles); entries beyond min(count, cap) are left at -1."""
    Kp = np.ascontiguousarray(Kp, np.int32)
    profile = np.full(cap, -1, np.int32)
    k0 = np.full(cap, -1, np.int32)
    count = _lib().dcp_reemit_tiles(len(Kp), Kp.ctypes.data_as(C.c_void_p), profile.ctypes.data_as(C.c_void_p),
                                    k0.ctypes.data_as(C.c_void_p), int(cap))
    return int(count), profile, k0


def cost_order_map(Q: int, W: int):
    """(cols int32[64 Q W], row stride in floats): where the cost-order copy of the emission rows keeps position k
    for the cost kernel of Q positions per lane and W wavefronts (csrc/host_logic.h dcp_cost_order_col)."""
    cols = np.zeros(64 * Q * W, np.int32)
    stride = int(_lib().dcp_cost_order_map(int(Q), int(W), cols.ctypes.data_as(C.c_void_p)))
    if stride <= 0:
        raise ValueError(f"no cost-order map for Q={Q}, W={W}")
    return cols, stride


ROW_CANON, ROW_COST_ORDER, ROW_PACK = 0, 1, 2


def row_lane_offsets(layout: int, Q: int, S: int, K: int):
    """(lanes that own a position below K, offsets uint32[lanes][chunks]): the byte offset inside an emission row
    that every lane of a cost kernel reads each chunk of its Q floats from, for a profile of K positions
    (csrc/dcp_types.h dcp_row_read_offset).  layout: ROW_CANON / ROW_COST_ORDER (64 lanes, chunks of four floats)
    or ROW_PACK (one group of S lanes, the separator first, one chunk)."""
    lanes, chunks = (S, 1) if layout == ROW_PACK else (64, (Q + 3) // 4)
    off = np.zeros((max(lanes, 1), max(chunks, 1)), np.uint32)
    real = int(_lib().dcp_row_lane_offsets(int(layout), int(Q), int(S), int(K), off.ctypes.data_as(C.c_void_p)))
    if real <= 0:
        raise ValueError(f"no cost kernel of layout {layout}, Q={Q}, S={S} takes K={K}")
    return real, off


def xcd_eighths_entry(b: int, n: int) -> int:
    """the entry of a list of n that workgroup b of a cost launch takes under the eighths (csrc/dcp_types.h
    dcp_xcd_eighths_entry): XCD b % 8 walks the (b % 8)-th contiguous eighth of the list"""
    L = _lib()
    L.dcp_xcd_eighths_entry_of.argtypes = [C.c_int, C.c_int]
    e = int(L.dcp_xcd_eighths_entry_of(int(b), int(n)))
    if e < 0:
        raise ValueError(f"no workgroup {b} in a launch of {n}")
    return e


PLACE_PLAIN, PLACE_EIGHTHS = 0, 1


def xcd_placement(workgroups: int, windows_per_profile: int, table_bytes: int, resident_per_xcd: int) -> int:
    """PLACE_PLAIN or PLACE_EIGHTHS: what a cost launch of that many windows in profile order does when nothing
    forces it (csrc/dcp_types.h dcp_xcd_placement)"""
    L = _lib()
    L.dcp_xcd_placement_of.argtypes = [C.c_int, C.c_int, C.c_int64, C.c_int]
    return int(L.dcp_xcd_placement_of(int(workgroups), int(windows_per_profile), int(table_bytes), int(resident_per_xcd)))


def plan_chunks(core_sizes, read_lengths, first_cells: float, later_cells: float, max_pairs: int, max_windows: int):
    """dcp_scan_run's cost batches: (chunks int32[n][4] = (p0, p1, s0, s1), windows int64[n]) -- profiles [p0, p1)
    x reads [s0, s1) -- for profiles and reads of these sizes (csrc/host_logic.h dcp_plan_chunks)."""
    L = _lib()
    K = np.ascontiguousarray(core_sizes, np.int32)
    R = np.ascontiguousarray(read_lengths, np.int32)
    cap = 64
    while True:
        chunks = np.zeros((cap, 4), np.int32)
        windows = np.zeros(cap, np.int64)
        n = C.c_int(0)
        rc = L.dcp_scan_plan_chunks(len(K), K.ctypes.data_as(C.c_void_p), len(R), R.ctypes.data_as(C.c_void_p),
                                    float(first_cells), float(later_cells), int(max_pairs), int(max_windows), cap,
                                    chunks.ctypes.data_as(C.c_void_p), windows.ctypes.data_as(C.c_void_p), C.byref(n))
        if rc == 20 and n.value > cap:  # DCP_ENOMEM: more chunks than room, their number is known now
            cap = n.value
            continue
        if rc:
            raise HipError(rc)
        return chunks[: n.value].copy(), windows[: n.value].copy()


PATH_FAST, PATH_LITERAL = 0, 1


def path_plan(kind: int, windows, B: int, budget: int, strict: bool = False, largest_chunk: int = 0, group_override: int = 0):
    """The memory plan of the path pass (csrc/path_plan.h dcp_plan_path) for windows = [(L, K, Kp, W, strip), ...]:
    a dict of G, blocked and, per window, in_blocks, blocks, replay_rows, ckpt_off, scratch_off and bytes."""
    cols = [np.ascontiguousarray([w[c] for w in windows], t) for c, t in enumerate((np.int32,) * 4 + (np.uint8,))]
    n = len(windows)
    out = {k: np.zeros(n, t) for k, t in (("in_blocks", np.int32), ("blocks", np.int32), ("replay_rows", np.int32),
                                          ("ckpt_off", np.int64), ("scratch_off", np.int64), ("bytes", np.int64))}
    G, blocked = C.c_int(0), C.c_int(0)
    rc = _lib().dcp_path_plan_of(int(kind), n, *(a.ctypes.data_as(C.c_void_p) for a in cols), int(B), int(budget),
                                 int(bool(strict)), int(largest_chunk), int(group_override),
                                 *(a.ctypes.data_as(C.c_void_p) for a in out.values()), C.byref(G), C.byref(blocked))
    if rc:
        raise HipError(rc)
    return dict(out, G=G.value, blocked=blocked.value)


ARENA_NONE, ARENA_TRELLIS, ARENA_TABLE = 0, 1, 2
NUM_CLASSES, NUM_PACK_SHAPES = 12, 11
PROBLEM = np.dtype([("profile", "i4"), ("L", "i4"), ("code_row", "i8"), ("xt_row", "i4"), ("out", "i4"),
                    ("trellis", "i8")])  # struct DcpProblem
PACK = np.dtype([("profile", "i4"), ("Lmax", "i4"), ("L", "i4", 16), ("xt_row", "i4", 16), ("out", "i4", 16),
                 ("code_row", "u4", 16)])  # struct DcpPack
_RANGES = (("c_begin", NUM_CLASSES + 1), ("c_wide", NUM_CLASSES), ("c_profiles", (NUM_CLASSES, 2)),
           ("pk_begin", NUM_PACK_SHAPES + 1), ("pg_begin", NUM_PACK_SHAPES + 1))
COST_KERNELS = ("none", "class", "narrow", "fused", "pack", "pack_lds")
COST_BRANCHES = ("class", "narrow", "pack")


def engine_core_size(K: int):
    """What the engine decides for a profile of K positions, without a device: (K, Kp, class, narrow, pack shape or -1),
    a row of stage_plan's `profiles`."""
    out = np.zeros(4, np.int32)
    rc = _lib().dcp_engine_core_size(int(K), out.ctypes.data_as(C.c_void_p))
    if rc:
        raise HipError(rc)
    return int(K), int(out[3]), int(out[0]), int(out[1]), int(out[2])


def engine_pack_shapes():
    """int32[11][2]: per pack shape the windows of a pack and the wavefronts of an LDS workgroup (0: none), the engine's"""
    out = np.zeros((NUM_PACK_SHAPES, 2), np.int32)
    for s in range(NUM_PACK_SHAPES):
        rc = _lib().dcp_engine_pack_shape(s, out[s].ctypes.data_as(C.c_void_p))
        if rc:
            raise HipError(rc)
    return out


def stage_plan(windows, profiles, seq_off, row_off=None, arena=ARENA_NONE, table_addr=None, pack=True, pack_lds=True,
               shapes=None):
    """The plan of a window list (csrc/stage_plan.h plan_stage) without an engine: windows int32[n][4] = (profile, read,
    start, stop), profiles rows of (K, Kp, class, narrow, pack shape), seq_off / row_off[nseq + 1] (row_off: as the
    engine lays the code rows out, by default), shapes as engine_pack_shapes() (the default).  A dict of problems
    (PROBLEM), packs (PACK), groups int32[..][2], the five range arrays, cells, arena_bytes and max_xt_row.  A refusal
    raises HipError with the engine's message."""
    L = _lib()
    vp = C.c_void_p
    w = np.ascontiguousarray(windows, np.int32).reshape(-1, 4)
    prof = np.ascontiguousarray(profiles, np.int32).reshape(-1, 5)
    so = np.ascontiguousarray(seq_off, np.int64)
    ro = np.ascontiguousarray(so + np.arange(len(so)) if row_off is None else row_off, np.int64)
    ta = None if table_addr is None else np.ascontiguousarray(table_addr, np.int64)
    sh = np.ascontiguousarray(engine_pack_shapes() if shapes is None else shapes, np.int32)
    assert len(ro) == len(so) >= 1 and sh.shape == (NUM_PACK_SHAPES, 2) and (ta is None or len(ta) == len(w))
    ranges = {k: np.zeros(shape, np.int32) for k, shape in _RANGES}
    cells, arena_bytes, max_xt, what = C.c_double(0), C.c_int64(0), C.c_int32(0), C.c_char_p()

    def call(sizes, problems, packs, groups):
        return L.dcp_stage_plan_of(
            len(w), w.ctypes.data_as(vp), len(prof), prof.ctypes.data_as(vp), len(so) - 1, so.ctypes.data_as(vp),
            ro.ctypes.data_as(vp), int(arena), None if ta is None else ta.ctypes.data_as(vp), int(bool(pack)),
            int(bool(pack_lds)), sh.ctypes.data_as(vp), sizes.ctypes.data_as(vp),
            *(None if a is None else a.ctypes.data_as(vp) for a in (problems, packs, groups)),
            *(a.ctypes.data_as(vp) for a in ranges.values()), C.byref(cells), C.byref(arena_bytes), C.byref(max_xt),
            C.byref(what))

    sizes = np.zeros(3, np.int64)
    rc = call(sizes, None, None, None)
    if rc:
        raise HipError(rc, (what.value or b"").decode())
    problems, packs, groups = np.zeros(sizes[0], PROBLEM), np.zeros(sizes[1], PACK), np.zeros((sizes[2], 2), np.int32)
    rc = call(sizes, problems, packs, groups)
    if rc:
        raise HipError(rc, (what.value or b"").decode())
    return dict(ranges, problems=problems, packs=packs, groups=groups, cells=cells.value, arena_bytes=arena_bytes.value,
                max_xt_row=max_xt.value)


def cost_schedule(plan, narrow: bool = True):
    """The launches of a cost pass over a staged list (csrc/stage_plan.h cost_schedule): plan holds the five range
    arrays (as stage_plan returns them); a list of dicts kernel, index, first, count, windows_per_profile, branch."""
    L = _lib()
    r = [np.ascontiguousarray(plan[k], np.int32) for k, _ in _RANGES]
    for a, (k, shape) in zip(r, _RANGES):
        assert a.shape == (shape if isinstance(shape, tuple) else (shape,)), k
    rows = np.zeros((2 * NUM_CLASSES + NUM_PACK_SHAPES + 1, 6), np.int32)
    n = L.dcp_cost_schedule_of(*(a.ctypes.data_as(C.c_void_p) for a in r), int(bool(narrow)), len(rows),
                               rows.ctypes.data_as(C.c_void_p))
    if n < 0 or n > len(rows):
        raise HipError(8)
    return [dict(kernel=COST_KERNELS[k], index=int(i), first=int(f), count=int(c), windows_per_profile=int(wpp),
                 branch=COST_BRANCHES[b]) for k, i, f, c, wpp, b in rows[:n]]


def trellis_arena(L, K):
    """(offsets int64[n], bytes): where the literal path pass puts the trellises of windows of L[i] rows and K[i]
    positions (csrc/stage_plan.h trellis_offsets)"""
    Ls, Ks = np.ascontiguousarray(L, np.int32), np.ascontiguousarray(K, np.int32)
    off = np.zeros(len(Ls), np.int64)
    total = _lib().dcp_trellis_arena_of(len(Ls), Ls.ctypes.data_as(C.c_void_p), Ks.ctypes.data_as(C.c_void_p),
                                        off.ctypes.data_as(C.c_void_p))
    if total < 0:
        raise HipError(8)
    return off, int(total)


WALK_HIT = np.dtype([("batch_index", "i4"), ("profile", "i4"), ("seq", "i4"), ("window", "i4"), ("start", "i4"),
                     ("stop", "i4"), ("lrt", "f4")])  # struct dcp_walk_hit


class ScanWalk:
    """dcp_scan_run's window walk without a GPU (include/deciphon_host.h dcp_scan_walk_*; the rules at
    csrc/scan_walk.h).  Windows are int32[n][4] = (profile, read, start, stop)."""

    COST, PATH = 0, 1

    def __init__(self, core_sizes, read_lengths):
        self.lib = _lib()
        K = np.ascontiguousarray(core_sizes, np.int32)
        R = np.ascontiguousarray(read_lengths, np.int32)
        self.h = self.lib.dcp_scan_walk_new(len(K), K.ctypes.data_as(C.c_void_p), len(R), R.ctypes.data_as(C.c_void_p))
        if not self.h:
            raise HipError(1)

    def __del__(self):
        if getattr(self, "h", None):
            self.lib.dcp_scan_walk_del(self.h)
            self.h = None

    def chunk_windows(self, chunk, windows: int):
        """-> (wins int32[windows][4], base int64[pairs + 1]) of chunk (p0, p1, s0, s1)."""
        c = np.ascontiguousarray(chunk, np.int32)
        wins = np.zeros((int(windows), 4), np.int32)
        base = np.zeros((int(c[1]) - int(c[0])) * (int(c[3]) - int(c[2])) + 1, np.int64)
        rc = self.lib.dcp_scan_walk_chunk_windows(self.h, c.ctypes.data_as(C.c_void_p), int(windows),
                                                  wins.ctypes.data_as(C.c_void_p), base.ctypes.data_as(C.c_void_p))
        if rc:
            raise HipError(rc)
        return wins, base

    def chunk_scored(self, chunk, base, hit_index, lrts) -> None:
        c = np.ascontiguousarray(chunk, np.int32)
        b = np.ascontiguousarray(base, np.int64)
        hi = np.ascontiguousarray(hit_index, np.int32)
        lr = np.ascontiguousarray(lrts, np.float32)
        rc = self.lib.dcp_scan_walk_chunk_scored(self.h, c.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p),
                                                 len(hi), hi.ctypes.data_as(C.c_void_p), lr.ctypes.data_as(C.c_void_p))
        if rc:
            raise HipError(rc)

    def all_pairs(self) -> None:
        self.lib.dcp_scan_walk_all_pairs(self.h)

    def waiting(self, which: int) -> int:
        return int(self.lib.dcp_scan_walk_waiting(self.h, which))

    def take(self, which: int) -> np.ndarray:
        p = C.c_void_p()
        n = int(self.lib.dcp_scan_walk_take(self.h, which, C.byref(p)))
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_int32)), (n, 4)).copy() if n else np.zeros((0, 4), np.int32)

    def cost_scored(self, hit_index, lrts) -> None:
        hi = np.ascontiguousarray(hit_index, np.int32)
        lr = np.ascontiguousarray(lrts, np.float32)
        rc = self.lib.dcp_scan_walk_cost_scored(self.h, len(hi), hi.ctypes.data_as(C.c_void_p),
                                                lr.ctypes.data_as(C.c_void_p))
        if rc:
            raise HipError(rc)

    def path_walked(self, is_hit, last_hit_pos) -> np.ndarray:
        """-> the hits (WALK_HIT records) as they stand before their pairs move on."""
        ih = np.ascontiguousarray(is_hit, np.uint8)
        lp = np.ascontiguousarray(last_hit_pos, np.int32)
        p = C.c_void_p()
        n = int(self.lib.dcp_scan_walk_path_walked(self.h, ih.ctypes.data_as(C.c_void_p), lp.ctypes.data_as(C.c_void_p),
                                                   C.byref(p)))
        if not n:
            return np.zeros(0, WALK_HIT)
        return np.frombuffer(C.string_at(p, n * WALK_HIT.itemsize), WALK_HIT).copy()

    def windows(self) -> int:
        return int(self.lib.dcp_scan_walk_windows(self.h))

    def take_queued(self) -> int:
        return int(self.lib.dcp_scan_walk_take_queued(self.h))


PRODUCT_STATS = ("rows", "runs", "peak_bytes", "file_bytes")


class ProductRuns:
    """The product rows of a scan in bounded memory, without a GPU (include/deciphon_host.h dcp_product_runs_*; the
    rules at csrc/product_runs.h): rows added in any order come out sorted by (profile, seq, window), equal keys in
    the order they were added, through sorted run files in `directory` once more than `budget_bytes` of text are held."""

    def __init__(self, directory, budget_bytes: int):
        self.lib = _lib()
        self.h = self.lib.dcp_product_runs_new(os.fsencode(directory), int(budget_bytes))
        if not self.h:
            raise HipError(8)

    def add(self, profile, seq, window, texts) -> None:
        """One call of add: rows (profile[i], seq[i], window[i], texts[i]), texts as bytes."""
        p, s, w = (np.ascontiguousarray(a, np.int32) for a in (profile, seq, window))
        assert len(p) == len(s) == len(w) == len(texts)
        t = (C.c_char_p * len(texts))(*texts)
        if rc := self.lib.dcp_product_runs_add(self.h, len(texts), p.ctypes.data_as(C.c_void_p),
                                               s.ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p), t):
            raise HipError(rc)

    def close(self, file) -> None:
        if rc := self.lib.dcp_product_runs_close(self.h, os.fsencode(file)):
            raise HipError(rc)

    def __len__(self):
        return int(self.lib.dcp_product_runs_num_rows(self.h))

    def row(self, i: int):
        """Row i of the closed file as bytes, without its newline; None out of range."""
        return self.lib.dcp_product_runs_row(self.h, int(i))

    def stats(self) -> dict:
        out = np.zeros(4, np.int64)
        n = self.lib.dcp_product_runs_stats(self.h, out.ctypes.data_as(C.c_void_p))
        assert n == len(PRODUCT_STATS)
        return {k: int(v) for k, v in zip(PRODUCT_STATS, out)}

    def free(self) -> None:
        if getattr(self, "h", None):
            self.lib.dcp_product_runs_del(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def unzip(K: int, L: int, xnodes: np.ndarray, nodes: np.ndarray):
    lib = _lib()
    xnodes = np.ascontiguousarray(xnodes, np.uint32)
    nodes = np.ascontiguousarray(nodes, np.uint16)
    cap = 2 * L + 2 * K + 16
    while True:
        ids = np.zeros(cap, np.int32)
        sizes = np.zeros(cap, np.int32)
        n = C.c_int(0)
        rc = lib.dcp_trellis_unzip(K, L, xnodes.ctypes.data_as(C.c_void_p), nodes.ctypes.data_as(C.c_void_p), cap,
                                   ids.ctypes.data_as(C.c_void_p), sizes.ctypes.data_as(C.c_void_p), C.byref(n))
        if rc == 20 and n.value > cap:  # DCP_ENOMEM: buffer too small, size is known now
            cap = n.value
            continue
        if rc:
            raise HipError(rc)
        return ids[: n.value].copy(), sizes[: n.value].copy()


def path_hit(state_ids, seqsizes):
    """-> (hit_start, hit_stop, begin_step, end_step, last_hit_pos) or None (c-core/thread.c:130-166)."""
    ids = np.ascontiguousarray(state_ids, np.int32)
    sizes = np.ascontiguousarray(seqsizes, np.int32)
    out = np.zeros(5, np.int32)
    ok = _lib().dcp_path_hit(len(ids), ids.ctypes.data_as(C.c_void_p), sizes.ctypes.data_as(C.c_void_p),
                             out.ctypes.data_as(C.c_void_p))
    return tuple(int(v) for v in out) if ok else None


def state_name(state_id: int) -> str:
    buf = C.create_string_buffer(8)
    _lib().dcp_state_name_of(int(state_id), buf)
    return buf.value.decode()


def state_is_mute(state_id: int) -> bool:
    return bool(_lib().dcp_state_is_mute_id(int(state_id)))


def lrt(null_loglik, alt_loglik) -> np.float32:
    return np.float32(_lib().dcp_lrt_of(float(null_loglik), float(alt_loglik)))


def random_thresholds(freq=None) -> np.ndarray:
    """The three cumulative thresholds of the random reads' generator from the frequencies of A, C, G, T (None:
    uniform), uint32 [3] (dcp_random_thresholds)."""
    t = np.zeros(3, np.uint32)
    f = None if freq is None else np.ascontiguousarray(freq, np.float32).reshape(4)
    rc = _lib().dcp_random_thresholds(None if f is None else f.ctypes.data_as(C.c_void_p), t.ctypes.data_as(C.c_void_p))
    if rc:
        raise HipError(rc)
    return t


def random_nt(seed: int, n: int, first_idx: int = 0, freq=None) -> np.ndarray:
    """Nucleotides first_idx .. first_idx + n of the random reads of `seed` (dcp_random_nt), uint8 indices 0..3: sequence
    s of a set of sequences of `length` nucleotides is random_nt(seed, length, s * length, freq), what
    Engine.set_random_sequences leaves as code rows."""
    t = random_thresholds(freq)
    out = np.zeros(int(n), np.uint8)
    rc = _lib().dcp_random_nt(int(seed) & (2**64 - 1), t.ctypes.data_as(C.c_void_p), int(first_idx), int(n),
                              out.ctypes.data_as(C.c_void_p))
    if rc:
        raise HipError(rc)
    return out


def lrt_evalue(lrt, mu, lam, z) -> float:
    """z * (1 - exp(-exp(-lam (lrt - mu)))), the Gumbel tail as dcp_lrt_evalue states it; NaN when mu is."""
    return float(_lib().dcp_lrt_evalue(float(lrt), float(mu), float(lam), float(z)))


def calib_mu_at(lens, mu, length) -> float:
    """mu at a window of `length` nucleotides from the rungs (lens[j], mu[j]) of a calibration over a ladder of read
    lengths: linear in ln length between the rungs whose mu is not NaN and beyond them (dcp_calib_mu_at)."""
    L = np.ascontiguousarray(lens, np.int32).reshape(-1)
    m = np.ascontiguousarray(mu, np.float32).reshape(-1)
    if len(L) != len(m):
        raise ValueError("lens and mu differ in length")
    return float(_lib().dcp_calib_mu_at(len(L), L.ctypes.data_as(C.c_void_p), m.ctypes.data_as(C.c_void_p), int(length)))


def decode_quasi_codon(epsilon: float, nucltp, codonm, nt) -> np.ndarray:
    """decoder_decode (c-core/decoder.c:38-58): codon (3 nucleotide indices) behind the 1..5 nucleotides nt."""
    a = np.ascontiguousarray(nucltp, np.float32)
    b = np.ascontiguousarray(codonm, np.float32)
    z = np.ascontiguousarray(nt, np.uint8)
    out = np.zeros(3, np.uint8)
    rc = _lib().dcp_decode_quasi_codon(float(epsilon), a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p),
                                       z.ctypes.data_as(C.c_void_p), len(z), out.ctypes.data_as(C.c_void_p))
    if rc:
        raise HipError(rc)
    return out


def gencode_amino(gencode_id: int, codon) -> str:
    c = np.ascontiguousarray(codon, np.uint8)
    r = _lib().dcp_gencode_amino_of(int(gencode_id), c.ctypes.data_as(C.c_void_p))
    return r.decode() if r != b"\0" else ""
