"""ctypes binding of include/deciphon_hip.h (the batched operator ABI)."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

TABLE_SIZE = 1364
NUM_TRANS = 8
NUM_XTRANS = 13
STRANDS = {"plus": 0, "both": 1}  # DCP_STRANDS_PLUS, DCP_STRANDS_BOTH


def strands_code(strands) -> int:
    """"plus" / "both" (or the C value itself) -> DCP_STRANDS_*; ValueError for a name that is neither."""
    if isinstance(strands, str):
        if strands not in STRANDS:
            raise ValueError(f"strands must be 'plus' or 'both', not {strands!r}")
        return STRANDS[strands]
    return int(strands)


class HipError(RuntimeError):
    def __init__(self, code: int, detail: str = ""):
        self.code = code
        msg = error_string(code)
        super().__init__(f"deciphon error {code}: {msg}" + (f" ({detail})" if detail else ""))


class Window(C.Structure):
    """struct dcp_hip_window: [start, stop) of sequence `seq` against `profile`."""

    _fields_ = [("profile", C.c_int32), ("seq", C.c_int32), ("start", C.c_int32), ("stop", C.c_int32)]


def library_path() -> str:
    # DECIPHON_HIP_LIBDIR: a build of the same library elsewhere (kernel experiments: make OUT=<dir> ...)
    return os.path.join(os.environ.get("DECIPHON_HIP_LIBDIR") or os.path.join(_HERE, "lib"), "libdeciphon_hip.so")


def load_library() -> C.CDLL:
    """Loads the HIP library; raises (never falls back) when it has not been built."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = library_path()
    if not os.path.exists(path):
        raise ImportError(f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(or make -C deciphon_amd/csrc); there is no CPU fallback")
    L = C.CDLL(path)
    vp, i32, f32p = C.c_void_p, C.c_int, C.POINTER(C.c_float)
    L.dcp_hip_device_count.restype = i32
    L.dcp_hip_new.argtypes = [i32]
    L.dcp_hip_new.restype = vp
    L.dcp_hip_del.argtypes = [vp]
    L.dcp_hip_del.restype = None
    L.dcp_hip_strerror.argtypes = [vp]
    L.dcp_hip_strerror.restype = C.c_char_p
    L.dcp_hip_add_profile.argtypes = [vp, i32, vp, vp, vp, vp, C.POINTER(i32)]
    L.dcp_hip_add_protein.argtypes = [vp, i32, vp, vp, vp, vp, vp, C.POINTER(i32)]
    L.dcp_hip_load_dcp.argtypes = [vp, C.c_char_p, i32, i32]
    L.dcp_hip_load_hmm.argtypes = [vp, C.c_char_p, i32, C.c_float, i32, i32]
    L.dcp_hip_set_epsilon.argtypes = [vp, C.c_float]
    L.dcp_hip_profile_epsilon.argtypes = [vp, i32]
    L.dcp_hip_profile_epsilon.restype = C.c_float
    L.dcp_hip_set_gencode.argtypes = [vp, i32]
    L.dcp_hip_profile_gencode.argtypes = [vp, i32]
    L.dcp_hip_dist_bytes.argtypes = [vp]
    L.dcp_hip_dist_bytes.restype = C.c_int64
    L.dcp_hip_profile_floats.argtypes = [vp, i32]
    L.dcp_hip_profile_floats.restype = C.c_int64
    L.dcp_hip_profile_read.argtypes = [vp, i32, vp, C.c_int64]
    L.dcp_hip_num_profiles.argtypes = [vp]
    L.dcp_hip_load_chunks.argtypes = [vp]
    L.dcp_hip_pool_bytes.argtypes = [vp]
    L.dcp_hip_pool_bytes.restype = C.c_int64
    L.dcp_hip_profile_core_size.argtypes = [vp, i32]
    L.dcp_hip_profile_accession.argtypes = [vp, i32]
    L.dcp_hip_profile_accession.restype = C.c_char_p
    L.dcp_hip_commit_profiles.argtypes = [vp]
    L.dcp_hip_clear_profiles.argtypes = [vp]
    L.dcp_hip_clear_profiles.restype = None
    L.dcp_hip_encode.argtypes = [C.c_char_p, C.c_int64, vp]
    L.dcp_hip_set_sequences.argtypes = [vp, i32, vp, vp]
    L.dcp_hip_set_sequences_strands.argtypes = [vp, i32, vp, vp, i32]
    L.dcp_hip_num_sequences.argtypes = [vp]
    L.dcp_hip_code_rows_read.argtypes = [vp, i32, vp, C.c_int64]
    L.dcp_hip_set_random_sequences.argtypes = [vp, i32, i32, C.c_uint64, vp]
    L.dcp_hip_calibrate.argtypes = [vp, i32, i32, C.c_uint64, vp, C.c_float]
    L.dcp_hip_profile_mu.argtypes = [vp, i32]
    L.dcp_hip_profile_mu.restype = C.c_float
    L.dcp_hip_profile_calib_excluded.argtypes = [vp, i32]
    L.dcp_hip_calib_lambda.argtypes = [vp]
    L.dcp_hip_calib_lambda.restype = C.c_float
    L.dcp_hip_calibrate_lengths.argtypes = [vp, i32, i32, vp, C.c_uint64, vp, C.c_float]
    L.dcp_hip_calib_num_lengths.argtypes = [vp]
    L.dcp_hip_calib_length.argtypes = [vp, i32]
    L.dcp_hip_profile_mu_rung.argtypes = [vp, i32, i32]
    L.dcp_hip_profile_mu_rung.restype = C.c_float
    L.dcp_hip_profile_calib_excluded_rung.argtypes = [vp, i32, i32]
    L.dcp_hip_profile_lambda.argtypes = [vp, i32]
    L.dcp_hip_profile_lambda.restype = C.c_float
    L.dcp_hip_profile_mu_at.argtypes = [vp, i32, C.c_int64]
    L.dcp_hip_profile_mu_at.restype = C.c_double
    L.dcp_hip_set_mode.argtypes = [vp, i32, i32]
    L.dcp_hip_set_xtrans_table.argtypes = [vp, i32, vp]
    L.dcp_hip_xtrans.argtypes = [i32, i32, i32, vp]
    L.dcp_hip_xtrans.restype = None
    L.dcp_hip_cost.argtypes = [vp, i32, vp, vp, vp]
    L.dcp_hip_cost_hits.argtypes = [vp, i32, vp, C.POINTER(i32), vp, vp]
    L.dcp_hip_cost_hits_begin.argtypes = [vp, i32, vp]
    L.dcp_hip_cost_hits_end.argtypes = [vp, C.POINTER(i32), vp, vp]
    L.dcp_hip_cost_bench.argtypes = [vp, i32, vp, i32, i32, f32p, C.POINTER(C.c_double), vp, vp]
    L.dcp_hip_stage.argtypes = [vp, i32, vp]
    L.dcp_hip_run_staged.argtypes = [vp, i32, f32p, C.POINTER(C.c_double)]
    L.dcp_hip_fetch_staged.argtypes = [vp, vp, vp]
    L.dcp_hip_last_cost_launches.argtypes = [vp, i32, vp]
    L.dcp_hip_path.argtypes = [vp, i32, vp]
    L.dcp_hip_path_redone.argtypes = [vp]
    L.dcp_hip_path_table_bytes.argtypes = [vp]
    L.dcp_hip_path_table_bytes.restype = C.c_int64
    L.dcp_hip_path_blocked.argtypes = [vp]
    L.dcp_hip_path_reserve.argtypes = [vp, C.c_int64]
    L.dcp_hip_path_nsteps.argtypes = [vp, i32]
    L.dcp_hip_path_steps.argtypes = [vp, i32, vp, vp]
    L.dcp_hip_path_steps_packed.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(C.c_int32)]
    L.dcp_hip_path_trellis.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(vp)]
    L.dcp_hip_path_score.argtypes = [vp, i32]
    L.dcp_hip_path_score.restype = C.c_float
    L.dcp_error_string.argtypes = [i32]
    L.dcp_error_string.restype = C.c_char_p
    _LIB = L
    return L


def error_string(code: int) -> str:
    try:
        s = load_library().dcp_error_string(int(code))
    except ImportError:
        return "?"
    return s.decode() if s else ""


def device_count() -> int:
    return int(load_library().dcp_hip_device_count())


def encode(data: str) -> np.ndarray:
    """dcp_batch_add's normalisation of one nucleotide string -> indices 0..3."""
    raw = data.encode()
    out = np.zeros(len(raw), dtype=np.uint8)
    rc = load_library().dcp_hip_encode(raw, len(raw), out.ctypes.data_as(C.c_void_p))
    if rc:
        raise HipError(rc)
    return out


def xtrans(seq_size: int, multi_hits: bool, hmmer3_compat: bool) -> np.ndarray:
    out = np.zeros(NUM_XTRANS, dtype=np.float32)
    load_library().dcp_hip_xtrans(int(seq_size), int(multi_hits), int(hmmer3_compat), out.ctypes.data_as(C.c_void_p))
    return out


def _p(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


def _f32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32)


class Engine:
    """One GPU's worth of resident profiles and reads (struct dcp_hip)."""

    def __init__(self, device: int = 0):
        self.lib = load_library()
        self.h = self.lib.dcp_hip_new(int(device))
        if not self.h:
            raise HipError(8, f"no usable HIP device {device}; there is no CPU fallback")
        self.device = int(device)
        self._seq_lens = []
        self._staged_n = 0
        self._path_shape = []

    def close(self):
        if getattr(self, "h", None):
            self.lib.dcp_hip_del(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc: int):
        if rc:
            raise HipError(rc, self.lib.dcp_hip_strerror(self.h).decode())

    # ---- profiles -------------------------------------------------------------
    def add_profile(self, K: int, trans, match, null, bg) -> int:
        trans, match, null, bg = _f32(trans), _f32(match), _f32(null), _f32(bg)
        assert trans.shape == (NUM_TRANS, K) and match.shape == (TABLE_SIZE, K)
        assert null.shape == (TABLE_SIZE,) and bg.shape == (TABLE_SIZE,)
        idx = C.c_int(-1)
        self._check(self.lib.dcp_hip_add_profile(self.h, K, _p(trans), _p(match), _p(null), _p(bg), C.byref(idx)))
        return idx.value

    def add_protein(self, K: int, node_trans, node_emission, BMk, null_lprob, bg_lprob) -> int:
        a = [_f32(v) for v in (node_trans, node_emission, BMk, null_lprob, bg_lprob)]
        assert a[0].shape == (K + 1, 7) and a[1].shape == (K + 1, TABLE_SIZE) and a[2].shape == (K,)
        idx = C.c_int(-1)
        self._check(self.lib.dcp_hip_add_protein(self.h, K, *[_p(v) for v in a], C.byref(idx)))
        return idx.value

    def load_dcp(self, path: str, first: int = 0, count: int = -1) -> None:
        self._check(self.lib.dcp_hip_load_dcp(self.h, os.fsencode(path), first, count))

    def load_hmm(self, path: str, gencode: int = 1, epsilon: float = 0.01, first: int = 0, count: int = -1) -> None:
        """Profiles [first, first + count) of a HMMER3 text file, their emission tables made on the GPU under
        translation table `gencode` and error rate `epsilon`: the pool load_dcp of the pressed file would leave."""
        self._check(self.lib.dcp_hip_load_hmm(self.h, os.fsencode(path), int(gencode), float(epsilon), first, count))

    def set_epsilon(self, epsilon: float) -> None:
        """Every profile again at error rate `epsilon`, on the GPU and in place: the pool load_hmm of the same files
        would leave at that rate.  Only for engines all of whose profiles came by load_hmm (DCP_EFUNCUSE otherwise)."""
        self._check(self.lib.dcp_hip_set_epsilon(self.h, float(epsilon)))

    def profile_epsilon(self, i: int) -> float:
        """The error rate profile i is at; NaN when it did not come by load_hmm."""
        return float(self.lib.dcp_hip_profile_epsilon(self.h, i))

    def set_gencode(self, gencode: int) -> None:
        """Every profile again under translation table `gencode`, each at its own error rate, without the files: the
        pool load_hmm of the same files would leave under that table.  Only for engines all of whose profiles came by
        load_hmm (DCP_EFUNCUSE otherwise); DCP_EGENCODEID for a table not held."""
        self._check(self.lib.dcp_hip_set_gencode(self.h, int(gencode)))

    def profile_gencode(self, i: int) -> int:
        """The translation table profile i is under; 0 when it did not come by load_hmm."""
        return int(self.lib.dcp_hip_profile_gencode(self.h, i))

    @property
    def dist_bytes(self) -> int:
        """HBM bytes of the distributions kept beside the pool for set_epsilon."""
        return int(self.lib.dcp_hip_dist_bytes(self.h))

    def profile_tables(self, i: int) -> np.ndarray:
        """Profile i as it lies in the pool (rows | trans | cost-order copy), copied: float32."""
        n = int(self.lib.dcp_hip_profile_floats(self.h, i))
        if n < 0:
            raise IndexError(i)
        out = np.empty(n, dtype=np.float32)
        self._check(self.lib.dcp_hip_profile_read(self.h, i, _p(out), n))
        return out

    @property
    def load_chunks(self) -> int:
        """Staging chunks the last load_dcp went through."""
        return self.lib.dcp_hip_load_chunks(self.h)

    @property
    def pool_bytes(self) -> int:
        """HBM bytes of the resident profile tables."""
        return int(self.lib.dcp_hip_pool_bytes(self.h))

    @property
    def num_profiles(self) -> int:
        return self.lib.dcp_hip_num_profiles(self.h)

    def core_size(self, i: int) -> int:
        return self.lib.dcp_hip_profile_core_size(self.h, i)

    def accession(self, i: int) -> str:
        s = self.lib.dcp_hip_profile_accession(self.h, i)
        return s.decode() if s else ""

    def commit(self) -> None:
        self._check(self.lib.dcp_hip_commit_profiles(self.h))

    def clear_profiles(self) -> None:
        """Drops every profile.  The C call returns no code: while cost batches are outstanding it does nothing, which
        shows here as DCP_EFUNCUSE."""
        self.lib.dcp_hip_clear_profiles(self.h)
        if getattr(self, "_pending", None) or self.num_profiles:
            raise HipError(8, self.lib.dcp_hip_strerror(self.h).decode())

    # ---- sequences ------------------------------------------------------------
    def set_sequences(self, seqs, strands="plus") -> None:
        """seqs: list of uint8 arrays of nucleotide indices 0..3.  strands="both" (dcp_hip_set_sequences_strands): the
        engine holds 2 len(seqs) sequences, 2s = seqs[s] and 2s + 1 = its reverse complement 3 - seqs[s][::-1], whose
        code rows the GPU writes from the one upload; windows address those indices."""
        code = strands_code(strands)
        seqs = [np.ascontiguousarray(s, dtype=np.uint8) for s in seqs]
        off = np.zeros(len(seqs) + 1, dtype=np.int64)
        np.cumsum([len(s) for s in seqs], out=off[1:])
        nt = np.concatenate(seqs) if seqs else np.zeros(0, dtype=np.uint8)
        nt = np.ascontiguousarray(nt)
        self._check(self.lib.dcp_hip_set_sequences_strands(self.h, len(seqs), _p(nt), _p(off), code))
        self._seq_lens = [len(s) for s in seqs for _ in range(2 if code == STRANDS["both"] else 1)]

    @staticmethod
    def _freq(freq):
        """freq[4] for the C call: None (uniform) stays NULL."""
        if freq is None:
            return None, None
        f = _f32(freq).reshape(4)
        return f, _p(f)

    def set_random_sequences(self, nseq: int, length: int, seed: int, freq=None) -> None:
        """nseq random sequences of `length` nucleotides whose code rows the GPU writes from a counter-based generator
        (dcp_hip_set_random_sequences): no read exists on the host or crosses the bus.  host.random_nt gives the same
        nucleotides.  freq: frequencies of A, C, G, T (None: uniform)."""
        keep, ptr = self._freq(freq)
        self._check(self.lib.dcp_hip_set_random_sequences(self.h, int(nseq), int(length), int(seed) & (2**64 - 1), ptr))
        self._seq_lens = [int(length)] * int(nseq)

    def calibrate(self, nseq: int, length: int, seed: int, freq=None, lam: float = 0.5) -> None:
        """Scores every profile against nseq random sequences of `length` nucleotides and fits the location mu of a
        Gumbel distribution of lrt at fixed lambda, all on the GPU (dcp_hip_calibrate).  lam = 0.5 is HMMER's conjectured
        ln 2 per bit, lrt being twice the log-odds in nats.  The random sequences stay resident: set yours again."""
        keep, ptr = self._freq(freq)
        self._check(self.lib.dcp_hip_calibrate(self.h, int(nseq), int(length), int(seed) & (2**64 - 1), ptr, float(lam)))
        self._seq_lens = [int(length)] * int(nseq)

    def profile_mu(self, i: int) -> np.float32:
        """The Gumbel location of profile i from the last calibrate(); NaN when it has none."""
        return np.float32(self.lib.dcp_hip_profile_mu(self.h, int(i)))

    def profile_calib_excluded(self, i: int) -> int:
        """Scores of profile i that the fit of the last calibrate() left out as not finite."""
        return int(self.lib.dcp_hip_profile_calib_excluded(self.h, int(i)))

    @property
    def calib_lambda(self) -> float:
        """lambda of the calibration in force as it was passed, 0 when it was fitted; NaN without one."""
        return float(self.lib.dcp_hip_calib_lambda(self.h))

    def calibrate_lengths(self, nseq: int, lengths, seed: int, freq=None, lam: float = 0.5) -> None:
        """calibrate() at every length of the increasing ladder `lengths` (dcp_hip_calibrate_lengths): rung j scores the
        reads of set_random_sequences(nseq, lengths[j], seed + j, freq).  lam = 0 fits one lambda per profile, common
        to its rungs, beside the locations.  The random sequences of the last rung stay resident: set yours again."""
        keep, ptr = self._freq(freq)
        lens = np.ascontiguousarray(lengths, np.int32).reshape(-1)
        self._check(self.lib.dcp_hip_calibrate_lengths(self.h, int(nseq), len(lens), _p(lens), int(seed) & (2**64 - 1), ptr, float(lam)))
        self._seq_lens = [int(lens[-1])] * int(nseq)

    @property
    def calib_lengths(self) -> tuple:
        """The ladder of the calibration in force: one length after calibrate(), () without a calibration."""
        return tuple(int(self.lib.dcp_hip_calib_length(self.h, j)) for j in range(self.lib.dcp_hip_calib_num_lengths(self.h)))

    def profile_mu_rung(self, i: int, j: int) -> np.float32:
        """The Gumbel location of profile i at rung j of calib_lengths; NaN when it has none."""
        return np.float32(self.lib.dcp_hip_profile_mu_rung(self.h, int(i), int(j)))

    def profile_calib_excluded_rung(self, i: int, j: int) -> int:
        """Scores of profile i at rung j that the fit left out as not finite."""
        return int(self.lib.dcp_hip_profile_calib_excluded_rung(self.h, int(i), int(j)))

    def profile_lambda(self, i: int) -> np.float32:
        """lambda of profile i: the one passed or, after lam = 0, the one fitted; NaN when it has none."""
        return np.float32(self.lib.dcp_hip_profile_lambda(self.h, int(i)))

    def profile_mu_at(self, i: int, length: int) -> float:
        """The Gumbel location of profile i at a window of `length` nucleotides: host.calib_mu_at of its rungs."""
        return float(self.lib.dcp_hip_profile_mu_at(self.h, int(i), int(length)))

    @property
    def num_sequences(self) -> int:
        """Internal sequences: the reads of the last set_sequences, twice as many on both strands."""
        return self.lib.dcp_hip_num_sequences(self.h)

    def code_rows(self, seq: int) -> np.ndarray:
        """The code rows of internal sequence `seq` as they lie in HBM, copied: uint32 [len + 1][8]
        (host.code_rows_of states them)."""
        if not 0 <= seq < len(self._seq_lens):
            raise IndexError(seq)
        out = np.empty((self._seq_lens[seq] + 1, 8), dtype=np.uint32)
        self._check(self.lib.dcp_hip_code_rows_read(self.h, int(seq), _p(out), len(out)))
        return out

    def set_mode(self, multi_hits: bool = True, hmmer3_compat: bool = False) -> None:
        self._check(self.lib.dcp_hip_set_mode(self.h, int(multi_hits), int(hmmer3_compat)))

    def set_xtrans_table(self, table) -> None:
        """table[rows][13]: caller-supplied special transitions for amino lengths 0..rows-1."""
        t = _f32(table).reshape(-1, NUM_XTRANS)
        self._check(self.lib.dcp_hip_set_xtrans_table(self.h, t.shape[0], _p(t)))

    # ---- the DP ---------------------------------------------------------------
    @staticmethod
    def _windows(windows):
        if isinstance(windows, np.ndarray):  # int32 [n][4] = (profile, seq, start, stop): no conversion
            a = np.ascontiguousarray(windows, dtype=np.int32).reshape(-1, 4)
            ptr = _p(a)
            ptr._keep = a
            return len(a), ptr
        n = len(windows)
        arr = (Window * max(n, 1))()
        for i, w in enumerate(windows):
            arr[i] = w if isinstance(w, Window) else Window(*w)
        return n, arr

    def cost(self, windows):
        """-> (null_cost[n], alt_cost[n]): viterbi_null / viterbi_cost of every window."""
        n, arr = self._windows(windows)
        nul = np.zeros(n, dtype=np.float32)
        alt = np.zeros(n, dtype=np.float32)
        self._check(self.lib.dcp_hip_cost(self.h, n, arr, _p(nul), _p(alt)))
        return nul, alt

    def cost_hits(self, windows):
        """-> (indices, lrt) of the windows whose lrt is finite and >= 0: the cost pass followed by
        process_window's filter (c-core/thread.c:118-121), both on the device."""
        n, arr = self._windows(windows)
        idx = np.zeros(max(n, 1), dtype=np.int32)
        lrt = np.zeros(max(n, 1), dtype=np.float32)
        nh = C.c_int(0)
        self._check(self.lib.dcp_hip_cost_hits(self.h, n, arr, C.byref(nh), _p(idx), _p(lrt)))
        return idx[: nh.value].copy(), lrt[: nh.value].copy()

    def cost_hits_begin(self, windows) -> None:
        """The first half of cost_hits: stages the windows, enqueues the kernels and returns while the GPU works.  Up to
        two batches may be outstanding; cost_hits_end() delivers the oldest."""
        n, arr = self._windows(windows)
        self._check(self.lib.dcp_hip_cost_hits_begin(self.h, n, arr))
        self._pending = getattr(self, "_pending", []) + [n]

    def cost_hits_end(self):
        n = self._pending.pop(0) if getattr(self, "_pending", None) else 0
        idx = np.zeros(max(n, 1), dtype=np.int32)
        lrt = np.zeros(max(n, 1), dtype=np.float32)
        nh = C.c_int(0)
        self._check(self.lib.dcp_hip_cost_hits_end(self.h, C.byref(nh), _p(idx), _p(lrt)))
        return idx[: nh.value].copy(), lrt[: nh.value].copy()

    def cost_bench(self, windows, warmup: int, reps: int):
        """-> (ms per launch, cells per launch, null_cost, alt_cost), timed with HIP events."""
        n, arr = self._windows(windows)
        nul = np.zeros(n, dtype=np.float32)
        alt = np.zeros(n, dtype=np.float32)
        ms = C.c_float(0)
        cells = C.c_double(0)
        self._check(self.lib.dcp_hip_cost_bench(self.h, n, arr, warmup, reps, C.byref(ms), C.byref(cells), _p(nul),
                                                _p(alt)))
        return ms.value, cells.value, nul, alt

    def stage(self, windows) -> None:
        """Copies the window list to HBM for run_staged() (measurement)."""
        n, arr = self._windows(windows)
        self._check(self.lib.dcp_hip_stage(self.h, n, arr))
        self._staged_n = n  # only once staged: fetch_staged sizes its buffers by it

    def run_staged(self, reps: int):
        """-> (HIP-event ms of `reps` cost-pass launches together, DP cells of one launch)."""
        ms = C.c_float(0)
        cells = C.c_double(0)
        self._check(self.lib.dcp_hip_run_staged(self.h, reps, C.byref(ms), C.byref(cells)))
        return ms.value, cells.value

    def fetch_staged(self):
        """-> (null_cost, alt_cost) of the last run_staged(reps > 0) over the staged list."""
        nul = np.zeros(self._staged_n, dtype=np.float32)
        alt = np.zeros(self._staged_n, dtype=np.float32)
        self._check(self.lib.dcp_hip_fetch_staged(self.h, _p(nul), _p(alt)))
        return nul, alt

    def last_cost_launches(self):
        """The launches of this engine's most recent cost pass (cost, cost_hits, cost_hits_begin -- of the batch begun
        last --, cost_bench, run_staged), in launch order: the dicts of host.cost_schedule, as the engine ran them."""
        from .host import COST_BRANCHES, COST_KERNELS

        n = self.lib.dcp_hip_last_cost_launches(self.h, 0, None)
        rows = np.zeros((max(n, 1), 5), np.int32)
        if n < 0 or self.lib.dcp_hip_last_cost_launches(self.h, len(rows), _p(rows)) != n:
            raise HipError(8)
        # a launch's branch follows from its kernel (csrc/stage_plan.cpp cost_schedule)
        branch = {"narrow": COST_BRANCHES[1], "pack": COST_BRANCHES[2], "pack_lds": COST_BRANCHES[2]}
        return [dict(kernel=COST_KERNELS[k], index=int(i), first=int(f), count=int(c), windows_per_profile=int(wpp),
                     branch=branch.get(COST_KERNELS[k], COST_BRANCHES[0])) for k, i, f, c, wpp in rows[:n]]

    def path_reserve(self, nbytes: int):
        """Set HBM aside for the path pass's DP tables now (its clearing overlaps what follows)."""
        self._check(self.lib.dcp_hip_path_reserve(self.h, int(nbytes)))

    @property
    def path_table_bytes(self) -> int:
        """The most HBM bytes of DP tables, checkpoints and replay scratch the last path() -- and the path_trellis()
        calls after it -- had placed at one time."""
        return int(self.lib.dcp_hip_path_table_bytes(self.h))

    @property
    def path_blocked(self) -> int:
        """How many windows of profiles beyond 4096 positions the last path() took a block at a time because their
        whole DP table exceeded the budget (DECIPHON_HIP_PATH_BUDGET_MB)."""
        return int(self.lib.dcp_hip_path_blocked(self.h))

    def path_steps_packed(self, i: int) -> np.ndarray:
        """Window i's steps of the last path() as the engine holds them (state id | emission length << 16), copied."""
        p, n = C.c_void_p(), C.c_int32(0)
        self._check(self.lib.dcp_hip_path_steps_packed(self.h, i, C.byref(p), C.byref(n)))
        if n.value == 0:
            return np.zeros(0, dtype=np.uint32)
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint32)), shape=(n.value,)).copy()

    def path(self, windows, trellis: bool = True):
        """viterbi_path + trellis_unzip -> list of dicts(score, state_ids, seqsizes[, xnodes, nodes]).
        The steps are read first (they come from the fast pass); trellis=True then asks for the
        packed back-pointers too, which makes the library run the literal pass for the batch."""
        n, arr = self._windows(windows)
        self._path_shape = []
        self._check(self.lib.dcp_hip_path(self.h, n, arr))
        # (K, L) of every window now: path_trellis() sizes its arrays by them whatever has changed since
        if isinstance(windows, np.ndarray):  # arr is then a bare pointer to the int32 [n][4] array
            w4 = np.asarray(windows, dtype=np.int32).reshape(-1, 4)
            self._path_shape = [(self.core_size(int(p)), int(b) - int(a)) for p, _, a, b in w4]
        else:
            self._path_shape = [(self.core_size(arr[i].profile), arr[i].stop - arr[i].start) for i in range(n)]
        self.path_redone = self.lib.dcp_hip_path_redone(self.h)
        out = []
        for i in range(n):
            ns = self.lib.dcp_hip_path_nsteps(self.h, i)
            ids = np.zeros(ns, dtype=np.int32)
            sizes = np.zeros(ns, dtype=np.int32)
            self._check(self.lib.dcp_hip_path_steps(self.h, i, _p(ids), _p(sizes)))
            out.append(dict(score=np.float32(self.lib.dcp_hip_path_score(self.h, i)), state_ids=ids, seqsizes=sizes))
        if not trellis:
            return out
        for i in range(n):
            out[i]["xnodes"], out[i]["nodes"] = self.path_trellis(i)
            # the literal pass has replaced the steps: they must be the very same path
            ns = self.lib.dcp_hip_path_nsteps(self.h, i)
            ids = np.zeros(ns, dtype=np.int32)
            sizes = np.zeros(ns, dtype=np.int32)
            self._check(self.lib.dcp_hip_path_steps(self.h, i, _p(ids), _p(sizes)))
            out[i]["literal_state_ids"], out[i]["literal_seqsizes"] = ids, sizes
            out[i]["literal_score"] = np.float32(self.lib.dcp_hip_path_score(self.h, i))
        return out

    def path_trellis(self, i: int):
        """-> (xnodes[L+1], nodes[(L+1)*K]) of window i of the last path(), copied; K and L as they were at that call.
        Any time after path(..., trellis=False); the library refuses (DCP_EFUNCUSE) once the profiles, sequences, mode
        or xtrans table have changed since."""
        xn, nd = C.c_void_p(), C.c_void_p()
        self._check(self.lib.dcp_hip_path_trellis(self.h, i, C.byref(xn), C.byref(nd)))
        K, L = self._path_shape[i]
        xnodes = np.ctypeslib.as_array(C.cast(xn, C.POINTER(C.c_uint32)), shape=(L + 1,)).copy()
        nodes = np.ctypeslib.as_array(C.cast(nd, C.POINTER(C.c_uint16)), shape=((L + 1) * K,)).copy()
        return xnodes, nodes
