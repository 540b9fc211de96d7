"""The lane-vocabulary conformance cases (tests/lanes/lane_cases.h) from Python: the two libraries behind one ABI, and
the seeded inputs of every case -- shared by tests/test_lane_ops_emul.py (the emulator against numpy, CPU) and
tests/test_gpu_lane_ops.py (the GPU's vocabulary against the emulator's, word for word).

A case takes `nin` per-lane input vectors of 64 W lanes, a row of scalars, read-only memory words shared by all vectors
and output memory words of its own per vector; it writes `nout` per-lane output vectors.  Everything is uint32 words;
floats travel as their bits."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from dcp_testlib import ROOT

LANES_DIR = os.path.join(ROOT, "tests", "lanes")
NSCAL = 4
SENTINEL = 0xA5A5A5A5  # what output memory holds before a case runs: a store that should not happen shows
TABLE_SIZE = 1364      # DCP_TABLE_SIZE: records of a pack's row resource
ROW_HDR = 4
COST_ORDER_HDR = 32

f32 = np.float32
INF = f32(np.inf)


def fbits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def ffrom(u):
    return np.ascontiguousarray(u, dtype=np.uint32).view(np.float32)


# every kind of fp32 an op can meet: both zeros, both infinities, a quiet NaN, denormals, ordinary and huge numbers
SPECIALS = ffrom(np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0x00000001, 0x80000001, 0x000B8AE2,
                           0x807FFFFF, 0x3F800000, 0xBF800000, 0x40600000, 0x7149F2CA, 0xF149F2CA, 0x00800000], np.uint32))


class Lib:
    def __init__(self, path):
        self.lib = C.CDLL(path)
        self.lib.lane_conf_name.restype = C.c_char_p
        self.lib.lane_conf_ops.restype = C.c_char_p
        self.lib.lane_conf_run.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_long,
                                           C.c_void_p, C.c_int]
        self.failed = None  # the first case that came back with an error: nothing is launched after it
        self.cases = {}
        for i in range(self.lib.lane_conf_count()):
            d = (C.c_int * 3)()
            assert self.lib.lane_conf_dims(i, d) == 0
            self.cases[self.lib.lane_conf_name(i).decode()] = (i, d[0], d[1], d[2], self.lib.lane_conf_ops(i).decode().split())

    def table(self):
        """name -> (W, nin, nout, [vocabulary names])"""
        return {n: c[1:] for n, c in self.cases.items()}

    def run(self, name, inp):
        """-> (out uint32[nvec][nout][64 W], omem uint32[nvec][omem_words])"""
        assert self.failed is None, f"{self.failed} failed before: no further case is run on this library"
        i, W, nin, nout, _ = self.cases[name]
        vin, scal, mem, omem = inp["in"], inp["scal"], inp["mem"], inp["omem"].copy()
        nvec = vin.shape[0]
        assert vin.shape == (nvec, nin, 64 * W) and vin.dtype == np.uint32 and vin.flags.c_contiguous
        assert scal.shape == (nvec, NSCAL) and scal.dtype == np.uint32 and scal.flags.c_contiguous
        assert mem.dtype == np.uint32 and mem.ndim == 1 and mem.size >= 1 and mem.flags.c_contiguous
        assert omem.dtype == np.uint32 and omem.shape[0] == nvec and omem.shape[1] % 4 == 0 and omem.shape[1] >= 4
        out = np.full((nvec, nout, 64 * W), 0xDEADBEEF, np.uint32)
        rc = self.lib.lane_conf_run(i, nvec, vin.ctypes.data, out.ctypes.data, scal.ctypes.data, NSCAL, mem.ctypes.data,
                                    mem.size, omem.ctypes.data, omem.shape[1])
        if rc != 0:
            self.failed = (name, rc)
        assert rc == 0, (name, rc)
        return out, omem


def make():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "emul"), "lanes"], check=True)


def emul_lib():
    make()
    return Lib(os.path.join(LANES_DIR, "liblane_conf_emul.so"))


def gpu_lib():
    make()
    return Lib(os.path.join(LANES_DIR, "liblane_conf_gpu.so"))


def same_words(a, b):
    """bit for bit, a NaN matching any NaN: -> bool array"""
    fa, fb = ffrom(a), ffrom(b)
    return (a == b) | (np.isnan(fa) & np.isnan(fb))


# ---- fp32 arithmetic as the vocabulary defines it -----------------------------------------------------------------
def fmin32(a, b):
    """min of two fp32 arrays: the number beside a NaN, and -0 below +0 (v_min_f32; lane_ops_emul.h em_fminf)"""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    a, b = np.broadcast_arrays(a, b)
    with np.errstate(invalid="ignore"):
        lo = np.where(a < b, a, b)
        tie = ffrom(fbits(a) | fbits(b)).reshape(a.shape)  # equal values: the same bits, or the two zeros -> -0
        r = np.where(a == b, tie, lo)
    return np.where(np.isnan(a), b, np.where(np.isnan(b), a, r)).astype(f32)


def fmin_reduce(x, axis=-1):
    x = np.moveaxis(np.asarray(x, f32), axis, 0)
    m = x[0]
    for v in x[1:]:
        m = fmin32(m, v)
    return m


def wave_tdd(DD):
    """put_tdd of one wavefront, DD float32[Q][64]: every lane its own positions but lane 0 its first, then a butterfly"""
    t = np.where(np.arange(64) == 0, f32(0), DD[0]).astype(f32)
    for q in range(1, DD.shape[0]):
        t = (t + DD[q]).astype(f32)
    for d in (32, 16, 8, 4, 2, 1):
        t = (t + t[np.arange(64) ^ d]).astype(f32)
    return t[63]


def could_bound(lo, tdd):
    """fma(-1e-4, |lo| + tdd, lo + tdd) in fp32 (one rounding: the product of two fp32 is exact in a double)"""
    lo, tdd = f32(lo), f32(tdd)
    return f32(np.float64(f32(-1e-4)) * np.float64(f32(abs(lo) + tdd)) + np.float64(f32(lo + tdd)))


def ulps(x, n):
    x = f32(x)
    for _ in range(abs(n)):
        x = np.nextafter(x, f32(np.inf) if n > 0 else f32(-np.inf), dtype=f32)
    return x


# ---- inputs --------------------------------------------------------------------------------------------------------
def costs(rng, shape, pinf=0.1):
    x = rng.uniform(0.0, 20.0, shape).astype(f32)
    x[rng.random(shape) < pinf] = INF
    return x


def mixed(rng, shape):
    """numbers of mixed magnitude and sign"""
    return (rng.standard_normal(shape) * 10.0 ** rng.integers(-3, 4, shape)).astype(f32)


def specials(rng, shape):
    return SPECIALS[rng.integers(0, len(SPECIALS), shape)]


def masks(rng, nvec, lanes):
    """0/1 vectors: empty, full, every single lane, then random ones of every density"""
    m = np.zeros((nvec, lanes), np.uint32)
    m[1] = 1
    for v in range(2, nvec):
        if v - 2 < lanes:
            m[v, v - 2] = 1
        else:
            m[v] = rng.random(lanes) < rng.random()
    return m


def pack(nvec, vecs, scal=None, mem=None, omem_words=4, lanes=64):
    """vecs: list of [nvec][lanes] arrays, float32 or uint32 -> the dict Lib.run takes"""
    lanes = vecs[0].shape[1] if vecs else lanes
    vin = np.zeros((nvec, len(vecs), lanes), np.uint32)
    for j, v in enumerate(vecs):
        assert v.shape == (nvec, lanes), (j, v.shape)
        vin[:, j] = fbits(v) if v.dtype == np.float32 else v.astype(np.uint32)
    s = np.zeros((nvec, NSCAL), np.uint32)
    for k, col in (scal or {}).items():
        col = np.asarray(col)
        s[:, k] = fbits(col) if col.dtype == np.float32 else col.astype(np.uint32)
    if mem is None:
        mem = np.arange(16, dtype=np.uint32)
    return {"in": vin, "scal": s, "mem": np.ascontiguousarray(mem, np.uint32),
            "omem": np.full((nvec, omem_words), SENTINEL, np.uint32)}


def min_in_every_lane(rng, lanes, lo, hi, least):
    """`lanes` vectors of values in [lo, hi), vector i with `least` in lane i"""
    x = rng.uniform(lo, hi, (lanes, lanes)).astype(f32)
    x[np.arange(lanes), np.arange(lanes)] = least
    return x


def fills(nvec):
    return np.array([0.0, np.inf, 2.5, -0.0, -3.0e30], f32)[np.arange(nvec) % 5]


def wave_min_vectors(rng):
    """the minimum in each of the 64 lanes in turn, duplicated minima, all +inf, denormals, the two zeros, -inf"""
    v = [min_in_every_lane(rng, 64, 1.0, 100.0, 0.5)]
    dup = rng.uniform(1.0, 100.0, (8, 64)).astype(f32)
    for r in range(8):
        dup[r, rng.choice(64, 2 + r % 3, replace=False)] = 0.25
    v.append(dup)
    v.append(np.full((1, 64), np.inf, f32))
    den = ffrom(rng.integers(2, 1 << 23, (8, 64)).astype(np.uint32)).copy()  # denormals, the least of them in any lane
    den[np.arange(8), rng.integers(0, 64, 8)] = ffrom(np.array([1], np.uint32))[0]
    v.append(den)
    zeros = np.zeros((8, 64), f32)  # +0 everywhere, -0 in one lane: the minimum is -0
    zeros[np.arange(8), [0, 1, 15, 16, 31, 32, 47, 63]] = f32(-0.0)
    v.append(zeros)
    one = np.full((4, 64), np.inf, f32)
    one[np.arange(4), [0, 17, 34, 63]] = [-np.inf, 3.0, -0.0, 1e-42]
    v.append(one)
    v.append(mixed(rng, (8, 64)))
    return np.concatenate(v)


def tdd_vectors(rng, Q, W, nvec, strip=False):
    """DD[Q], m_last, i_last, d_last, m_all of nvec rows and what get_e_could[_row] must say: the d a wavefront
    published stands a few ulps to either side of the bound, in a wavefront chosen per row, and every third row has the
    numbers of delete_run_cases.cancelling_run (E = -996.25 against a tdd of about +1000)"""
    lanes = 64 * W
    DD = np.zeros((nvec, Q, lanes), f32)
    ml, il = mixed(rng, (nvec, lanes)), mixed(rng, (nvec, lanes))
    dl = np.zeros((nvec, lanes), f32)
    mall = np.zeros((nvec, lanes), f32)
    floor_e = np.zeros(nvec, f32)
    E = np.zeros(nvec, f32)
    could = np.zeros(nvec, bool)
    for v in range(nvec):
        cancel = v % 3 == 0
        if cancel:
            DD[v] = (1000.0 / (64 * Q) * rng.uniform(0.5, 1.5, (Q, lanes))).astype(f32)
            mall[v] = rng.uniform(-900.0, 50.0, lanes)
            mall[v, rng.integers(0, lanes)] = -996.25
        else:
            DD[v] = (rng.random((Q, lanes)) * 10.0 ** rng.uniform(-4, 1.5, (Q, lanes))).astype(f32)
            mall[v] = rng.uniform(0.0, 30.0, lanes)
        DD[v, 0, ::64] = 1.0e6  # the first position of a wavefront is not part of its sum
        tdd = np.array([wave_tdd(DD[v][:, 64 * w : 64 * w + 64]) for w in range(W)], f32)
        m = fmin_reduce(mall[v])
        floor_e[v] = m + f32(rng.choice([-3.0, 5.0])) if strip else m
        lo = min(m, floor_e[v]) if strip else m
        bound = np.array([could_bound(lo, t) for t in tdd], f32)
        wt, side = v % W, (v // W) % 2 == 0
        for w in range(W):
            # bound < d decides: a wavefront that cannot be lowered published a d at or below its bound
            d = ulps(bound[w], 3 if side else -3) if w == wt else f32(bound[w] - abs(bound[w]) * 0.5 - 1.0)
            dl[v, 64 * w + 63] = d
        dl[v, np.arange(lanes) % 64 != 63] = rng.uniform(-5.0, 5.0, lanes - W)
        E[v], could[v] = m, side
    vecs = [DD[:, q] for q in range(Q)] + [ml, il, dl, mall]
    return vecs, floor_e, E, could


def case_inputs(name, W, nin, nout, seed=20260):
    """the seeded inputs of a case -> dict for Lib.run, with "expect" where the builder knows the answer"""
    rng = np.random.default_rng([seed, sum(name.encode()) * 131 + len(name)])
    lanes = 64 * W
    fam = name.split("<")[0].split("/")[0]
    targs = [int(x) for x in re.findall(r"\d+", name.split("/")[0].split("<")[1])] if "<" in name else []
    ctx = name.split("/")[1] if "/" in name else None

    if fam == "elem_f":
        n = len(SPECIALS)
        a = np.repeat(SPECIALS, n)
        b = np.tile(SPECIALS, n)  # every ordered pair of the special values
        k = -(-len(a) // 64)
        a = np.resize(a, (k, 64)).astype(f32)
        b = np.resize(b, (k, 64)).astype(f32)
        a = np.concatenate([a, mixed(rng, (8, 64)), specials(rng, (8, 64))])
        b = np.concatenate([b, mixed(rng, (8, 64)), specials(rng, (8, 64))])
        c = np.concatenate([specials(rng, (k, 64)), mixed(rng, (8, 64)), specials(rng, (8, 64))])
        b[k + 1] = a[k + 1]  # equal numbers
        return pack(len(a), [a, b, c], {0: fills(len(a))})
    if fam == "elem_u":
        nvec = 40
        a = rng.integers(0, 1 << 32, (nvec, 64), dtype=np.uint64).astype(np.uint32)
        b = rng.integers(0, 1 << 32, (nvec, 64), dtype=np.uint64).astype(np.uint32)
        b[:, ::5] = a[:, ::5]
        a[0], b[0] = 0, 0xFFFFFFFF
        c = np.where(rng.random((nvec, 64)) < 0.5, a, b)
        return pack(nvec, [a, b, c], {0: np.arange(nvec) % 32, 1: rng.integers(0, 1 << 32, nvec, dtype=np.uint64)})
    if fam == "shift_up":
        nvec = 20
        a = np.concatenate([mixed(rng, (10, 64)), specials(rng, (10, 64))])
        b = np.concatenate([mixed(rng, (10, 64)), specials(rng, (10, 64))])
        return pack(nvec, [a, b], {0: fills(nvec)})
    if fam in ("shift_keep", "group1_keep"):
        nvec = 20
        keep = mixed(rng, (nvec, 64))
        keep[:, 0] = fills(nvec)
        return pack(nvec, [costs(rng, (nvec, 64)), keep, costs(rng, (nvec, 64), 0.0)])
    if fam == "seg_shift":
        nvec = 12
        return pack(nvec, [mixed(rng, (nvec, lanes)), mixed(rng, (nvec, lanes)), specials(rng, (nvec, lanes))])
    if fam == "wave_min":
        a = wave_min_vectors(rng)
        nvec = len(a)
        b = np.full((nvec, 64), -0.0, f32)  # a + (-0) is a, to the bit
        b[-8:] = mixed(rng, (8, 64))
        if ctx == "twice":
            b = np.concatenate([wave_min_vectors(rng)[nvec // 2 :], wave_min_vectors(rng)[: nvec // 2]])
        return pack(nvec, [a, b, mixed(rng, (nvec, 64))])
    if fam == "wave_minu":
        a = rng.integers(1000, 1 << 32, (64 + 12, 64), dtype=np.uint64).astype(np.uint32)
        a[np.arange(64), np.arange(64)] = 7  # the minimum in each lane in turn
        for r in range(64, 72):
            a[r, rng.choice(64, 3, replace=False)] = 99  # duplicated minima
        a[72] = 0xFFFFFFFF
        a[73] = 0
        a[74, 63] = 0
        a[75, 0] = 0x80000000
        nvec = len(a)
        b = np.zeros((nvec, 64), np.uint32)
        b[70:] = rng.integers(0, 1 << 31, (nvec - 70, 64))
        if ctx == "twice":
            b = a[::-1].copy()
        return pack(nvec, [a, b, rng.integers(0, 1 << 32, (nvec, 64), dtype=np.uint64).astype(np.uint32)])
    if fam == "add_quad0_x5":
        nvec = 24
        v = [np.concatenate([mixed(rng, (16, 64)), specials(rng, (8, 64))]) for _ in range(11)]
        return pack(nvec, v)
    if fam == "groups":
        a = np.concatenate([min_in_every_lane(rng, 64, 1.0, 100.0, 0.5), specials(rng, (8, 64)), mixed(rng, (8, 64))])
        z = np.zeros((4, 64), f32)  # the two zeros: -0 in one lane of a group, in either DPP row of a group of 32
        z[np.arange(4), [1, 18, 37, 63]] = f32(-0.0)
        a = np.concatenate([a, z])
        nvec = len(a)
        b = np.full((nvec, 64), -0.0, f32)
        b[64:80] = mixed(rng, (16, 64))
        return pack(nvec, [a, b])
    if fam == "votes":
        nvec = 80
        m = masks(rng, nvec, 64)
        ub = rng.integers(0, 1 << 32, (nvec, 64), dtype=np.uint64).astype(np.uint32)
        return pack(nvec, [m, mixed(rng, (nvec, 64)), ub, mixed(rng, (nvec, 64))], {0: np.arange(nvec) % 64})
    if fam == "lane_policy":
        nvec = 70
        t = np.zeros((nvec, 128), np.uint32)
        t[:, :64] = masks(rng, nvec, 64) * 3 + 4 * rng.integers(0, 100, (nvec, 64))  # bit 0 is the predicate
        keys = rng.integers(-1000, 1000, (nvec, 64)).astype(np.int32)
        keys[np.arange(64), np.arange(64)] = 5000  # the maximum in each lane in turn
        keys[64] = -7
        t[:, 64:] = keys.view(np.uint32)
        return pack(nvec, [], {0: np.arange(nvec) * 128}, mem=t.reshape(-1))
    if fam == "group_exchange":
        nvec = 24
        a, b, X = mixed(rng, (nvec, lanes)), mixed(rng, (nvec, lanes)), mixed(rng, (nvec, lanes))
        for v in range(min(nvec, 2 * W)):  # the minimum in the last and in the first lane of each wavefront
            b[v, 64 * (v // 2) + (63 if v % 2 else 0)] = -1.0e9
        b[-1] = np.inf
        ua = rng.integers(5, 1 << 32, (nvec, lanes), dtype=np.uint64).astype(np.uint32)
        for v in range(min(nvec, 2 * W)):
            ua[v, 64 * (v // 2) + (63 if v % 2 else 0)] = 2
        m = masks(rng, nvec, lanes)
        m[2 : 2 + 2 * W] = 0
        for v in range(2 * W):  # a single vote in the first or last lane of one wavefront
            m[2 + v, 64 * (v // 2) + (63 if v % 2 else 0)] = 1
        every = np.zeros((nvec, lanes), np.uint32)  # empty, or set in every wavefront
        for v in range(0, nvec, 2):
            every[v, np.arange(W) * 64 + rng.integers(0, 64, W)] = 1
        return pack(nvec, [a, b, ua, m, X, every], {0: fills(nvec)})
    if fam == "group_rec":
        nvec = 12
        return pack(nvec, [mixed(rng, (nvec, lanes)) for _ in range(7)], {0: np.arange(nvec) % 2, 1: (np.arange(nvec) // 2) % 3})
    if fam == "group_tdd":
        nvec = 8 * W
        vecs, _, E, could = tdd_vectors(rng, targs[0], W, nvec)
        r = pack(nvec, vecs, {0: np.arange(nvec) % 2})
        r["expect"] = (E, could)
        return r
    if fam == "group_tdd_strip":
        nvec = 8 * W
        vecs, floor_e, E, could = tdd_vectors(rng, targs[0], W, nvec, strip=True)
        r = pack(nvec, vecs, {0: np.arange(nvec) % 2, 1: np.arange(nvec) % 8, 2: floor_e, 3: (np.arange(nvec) // 2) % 2})
        r["expect"] = (E, could)
        return r
    if fam == "stash":
        nvec = 6
        return pack(nvec, [np.concatenate([mixed(rng, (4, lanes)), specials(rng, (2, lanes))]) for _ in range(nin)])
    if fam == "pack_stash":
        nvec = 6
        return pack(nvec, [np.concatenate([mixed(rng, (4, 64)), specials(rng, (2, 64))]) for _ in range(nin)])
    if fam == "load_store_q":
        Q, nvec = targs[0], 6
        mem = mixed(rng, 64 * Q + 32)
        return pack(nvec, [mixed(rng, (nvec, 64)) for _ in range(Q)], {0: 4 * (np.arange(nvec) % 5), 1: 4 * (np.arange(nvec) % 3)},
                    mem=fbits(mem), omem_words=64 * Q + 16)
    if fam == "row_q":
        Q, nvec = targs[0], 6
        stride = ROW_HDR + 64 * Q
        mem = mixed(rng, 3 * stride)
        # rows 0..2 of a resource that ends with row 2: its last lane reads up to the last dword
        return pack(nvec, [], {0: np.full(nvec, 12 * stride), 1: 4 * stride * (np.arange(nvec) % 3)}, mem=fbits(mem))
    if fam == "row_chunks":
        Q, nvec = targs[0], 8
        ordered = np.arange(nvec) % 2
        stride = np.where(ordered == 1, COST_ORDER_HDR, ROW_HDR) + 64 * Q * W
        mem = mixed(rng, 3 * (COST_ORDER_HDR + 64 * Q * W))
        return pack(nvec, [], {0: 12 * stride, 1: 4 * stride * ((np.arange(nvec) // 2) % 3), 2: ordered}, mem=fbits(mem), lanes=lanes)
    if fam in ("pack_q", "code_row"):
        Q = targs[0] if targs else 1
        Kp = 512 if fam == "pack_q" else 64
        rows = TABLE_SIZE * (Kp + ROW_HDR) if fam == "pack_q" else 8
        at = -(-rows // 8) * 8
        ncode, have = 40, 48  # code rows of the resource, and rows that lie in memory behind them (never zero)
        mem = np.concatenate([fbits(mixed(rng, at)), rng.integers(1, 1 << 20, have * 8).astype(np.uint32)])
        nvec = 6
        e = np.arange(64)
        col = np.zeros((nvec, 64), np.uint32)  # 0: the header; else the column of the lane in its group of S
        for v, S in zip(range(1, nvec), (4, 8, 16, 32, 64)):
            col[v] = np.where(e % S == 0, 0, 16 + 4 * Q * (e % S - 1))
        if fam == "pack_q":
            idx = rng.integers(0, TABLE_SIZE, (nvec, 64)).astype(np.uint32)
            idx[:, 0], idx[:, 63] = 0, TABLE_SIZE - 1
        else:
            idx = rng.integers(0, ncode, (nvec, 64)).astype(np.uint32)
            idx[:, 3], idx[:, 4], idx[:, 5], idx[:, 63] = ncode - 1, ncode, ncode + 5, ncode + 5
            idx[1] = ncode
        return pack(nvec, [col, idx], {0: np.full(nvec, Kp), 1: np.full(nvec, at), 2: np.full(nvec, ncode)}, mem=mem)
    if fam == "cols":
        nvec = 6
        return pack(nvec, [rng.integers(0, 200, (nvec, 64)).astype(np.uint32)], {0: np.arange(nvec) * 3},
                    mem=fbits(mixed(rng, 256)))
    if fam == "nodes":
        Q, nvec = targs[0], 10
        K = rng.integers(1, 64 * Q + 1, nvec)
        K[0], K[1], K[2] = 64 * Q, 1, 64 * Q - 1
        return pack(nvec, [rng.integers(0, 1 << 32, (nvec, 64), dtype=np.uint64).astype(np.uint32) for _ in range(Q)], {0: K},
                    omem_words=32 * Q)
    if fam == "lds":
        N, nvec, n = targs[0], 6, 1024
        return pack(nvec, [(N * rng.integers(0, (n - N) // N + 1, (nvec, 64))).astype(np.uint32)], {0: np.full(nvec, n)},
                    mem=fbits(mixed(rng, n)))
    if fam == "lane_mem":
        nvec = 8
        mem = fbits(mixed(rng, 500))
        perm = np.stack([rng.permutation(64) for _ in range(nvec)]).astype(np.uint32)
        v = [rng.integers(0, 500, (nvec, 64)).astype(np.uint32), perm, masks(rng, nvec, 64)]
        v += [mixed(rng, (nvec, 64)) for _ in range(7)]
        return pack(nvec, v, {0: rng.integers(0, 1 << 32, nvec, dtype=np.uint64), 1: mixed(rng, nvec)}, mem=mem, omem_words=144)
    raise KeyError(name)
