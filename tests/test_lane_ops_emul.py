"""CPU: the wave emulator's lane vocabulary (tests/emul/lane_ops_emul.h) op by op against plain numpy definitions
written here -- the specification that tests/test_gpu_lane_ops.py then holds the GPU's vocabulary
(deciphon_amd/csrc/lane_ops_gpu.h) to, from the same cases (tests/lanes/lane_cases.h) and the same seeded inputs
(tests/lane_conf_cases.py).  Every test_emul_* suite assumes the two vocabularies mean the same; this file and its GPU
twin are where that is checked directly.

Also the completeness guard: every DCP_FN function and every Group member that lane_ops_gpu.h declares is covered by a
case of the table, or exempt because it has no result that could be observed."""
import os
import re

import numpy as np
import pytest

import lane_conf_cases as lc
from dcp_testlib import ROOT
from lane_conf_cases import COST_ORDER_HDR, INF, ROW_HDR, SENTINEL, f32, fbits, ffrom, fmin32, fmin_reduce

# ops without an observable result: nothing a case could compare
EXEMPT = {
    "sched_fence": "a scheduling barrier for the compiler: no value, no store",
    "wave_priority": "sets the wavefront's issue priority (s_setprio): no value, no store",
    "note_fallback": "empty on the GPU: only the emulator counts with it (emul_fallback_rows)",
}


@pytest.fixture(scope="module")
def em():
    return lc.emul_lib()


def names():
    """the case names, from the table in lane_cases.h as the built library reports it"""
    return sorted(lc.emul_lib().table())


def declared_ops():
    """names declared in lane_ops_gpu.h: free DCP_FN functions and members of Group / DcpLanesWave"""
    src = open(os.path.join(ROOT, "deciphon_amd", "csrc", "lane_ops_gpu.h")).read()
    src = re.sub(r"//[^\n]*", "", src)
    found = set(re.findall(r"DCP_FN\s+(?:static\s+)?[\w:<>,\s\*&]*?[\s\*&](\w+)\s*\(", src))
    return found


def test_every_declared_op_has_a_case(em):
    ops = declared_ops()
    # the parse sees what it should: a free function, a template, a Group member, a static member of the lane policy
    assert {"lmin", "load_row_q", "get_e_could_row", "max_of", "pack_unstash_wait", "wave_priority", "dcp_stash"} <= ops
    assert len(ops) > 100
    covered = set()
    for W, nin, nout, case_ops in em.table().values():
        covered |= set(case_ops)
    assert covered <= ops, sorted(covered - ops)  # the table names only what exists
    assert not (covered & set(EXEMPT))
    assert set(EXEMPT) <= ops
    missing = ops - covered - set(EXEMPT)
    assert not missing, sorted(missing)
    assert all(len(reason) > 10 for reason in EXEMPT.values())


def test_the_table_has_the_shapes_the_kernels_instantiate(em):
    t = set(em.table())
    for Q in (1, 2, 3, 4, 5, 6, 7, 8, 10):
        assert {f"stash<{Q},1>", f"stash<{Q},2>", f"load_store_q<{Q}>", f"row_q<{Q}>"} <= t
    for Q in (5, 6, 7, 8, 10):
        assert {f"row_chunks<{Q},1>", f"row_chunks<{Q},2>"} <= t
    for Q in (1, 2, 3, 4, 6, 8):
        assert f"pack_q<{Q}>" in t
    for S in (4, 8, 16, 32):
        assert f"groups<{S}>" in t
    for W in (1, 2, 4, 8):
        assert f"group_exchange<{W}>" in t
    for W in (2, 4, 8):
        assert {f"seg_shift<{W}>", f"group_rec<{W}>"} <= t
    for op in ("wave_min", "wave_minu", "add_quad0_x5", "pack_stash<1>", "pack_stash<2>", "pack_stash<3>", "pack_stash<4>"):
        assert {f"{op}/valu", f"{op}/load", f"{op}/twice"} <= t  # the assembly-bearing ops in three contexts


def shift_up(x, fill):
    """lane e takes lane e - 1, lane 0 the fill (fill: per vector)"""
    r = np.roll(x, 1, axis=-1)
    r[..., 0] = fill
    return r


def seg_shift_up(x, fill):
    """the same per wavefront: the first lane of each takes its own lane of `fill`"""
    r = np.roll(x, 1, axis=-1)
    r[..., ::64] = fill[..., ::64]
    return r


def group_of(x, S):
    return x.reshape(x.shape[0], -1, S)


def expected(name, W, inp):
    """-> ({output j: float32 or uint32 [nvec][lanes] or [nvec] (uniform)}, omem or None) by plain numpy"""
    vin, scal, mem = inp["in"], inp["scal"], inp["mem"]
    nvec, lanes = vin.shape[0], 64 * W
    F = lambda j: ffrom(vin[:, j]).reshape(nvec, lanes)
    U = lambda j: vin[:, j]
    sf = lambda s: ffrom(scal[:, s])
    su = lambda s: scal[:, s]
    memf = ffrom(mem)
    fam = name.split("<")[0].split("/")[0]
    targs = [int(x) for x in re.findall(r"\d+", name.split("/")[0].split("<")[1])] if "<" in name else []
    ctx = name.split("/")[1] if "/" in name else None
    e = np.arange(lanes)
    omem = inp["omem"].copy()
    with np.errstate(all="ignore"):
        if fam == "elem_f":
            a, b, c = F(0), F(1), F(2)
            s0 = sf(0)[:, None]
            return {0: fmin32(a, b), 1: fmin32(b, a), 2: fmin32(fmin32(a, b), c), 3: fmin32(fmin32(c, b), a),
                    4: (a < b).astype(np.uint32), 5: (a == b).astype(np.uint32), 6: np.where(a < b, a, c), 7: -a, 8: a + b,
                    9: np.broadcast_to(s0, a.shape), 10: s0 + a, 11: a + s0}, None
        if fam == "elem_u":
            a, b, c = U(0), U(1), U(2)
            return {9: ((a < b) & (a == c)).astype(np.uint32), 10: ((a < b) | (a == c)).astype(np.uint32),
                    11: (a != b).astype(np.uint32), 0: (a < b).astype(np.uint32), 1: (a == b).astype(np.uint32), 2: np.where(a < b, a, b), 3: np.minimum(a, b),
                    4: np.maximum(a, b), 5: a >> su(0)[:, None], 6: np.broadcast_to(su(1)[:, None], a.shape),
                    7: np.broadcast_to(e.astype(np.uint32), a.shape), 8: a + b}, None
        if fam == "shift_up":
            a, b, fill = F(0), F(1), sf(0)
            y = shift_up(a + b, fill)
            return {0: shift_up(a, fill), 1: y, 2: shift_up(a, f32(0)), 3: shift_up(y, f32(0)), 4: y}, None
        if fam in ("shift_keep", "group1_keep"):
            x, keep, step = F(0).copy(), F(1).copy(), F(2)
            for _ in range(50):
                keep = shift_up(x, keep[:, 0])
                s = keep
                x = fmin32(s + step, x)
            out = {0: s, 1: keep}
            out[2] = x if fam == "shift_keep" else np.broadcast_to(e.astype(np.uint32), x.shape)
            return out, None
        if fam == "seg_shift":
            a, b, fill = F(0), F(1), F(2)
            return {0: seg_shift_up(a, fill), 1: seg_shift_up(a + b, fill), 2: np.broadcast_to((e % 64 == 0).astype(np.uint32), a.shape),
                    3: np.broadcast_to((e % 64 == 63).astype(np.uint32), a.shape), 4: np.broadcast_to(e.astype(np.uint32), a.shape)}, None
        if fam == "wave_min":
            if ctx == "valu":
                return {0: fmin_reduce(F(0) + F(1))}, None
            m = fmin_reduce(F(0))
            if ctx == "load":
                return {0: m}, None
            return {0: m, 1: fmin_reduce(fmin32(F(1), m[:, None] + F(2)))}, None
        if fam == "wave_minu":
            if ctx == "valu":
                return {0: (U(0) + U(1)).min(axis=1)}, None
            m = U(0).min(axis=1)
            if ctx == "load":
                return {0: m}, None
            return {0: m, 1: np.maximum(U(1), m[:, None] + U(2)).min(axis=1)}, None
        if fam == "add_quad0_x5":
            s = [F(t) + F(10) if ctx == "valu" else F(t) for t in range(5)]
            q = [F(5 + t) + F(10) if ctx == "valu" else F(5 + t) for t in range(5)]
            r = [s[t] + q[t][:, e & ~3] for t in range(5)]
            out = {t: r[t] for t in range(5)}
            if ctx == "twice":
                out.update({5 + t: s[t] + r[t][:, e & ~3] for t in range(5)})
            return out, None
        if fam == "groups":
            S = targs[0]
            out = {}
            for k, x in enumerate((F(0), F(0) + F(1))):
                g = group_of(x, S)
                out[k] = np.repeat(fmin_reduce(g), S, axis=-1).reshape(x.shape)
                out[2 + k] = np.repeat(fmin32(g[..., 0], g[..., 1]), S, axis=-1).reshape(x.shape)
                out[4 + k] = x[:, e & ~(S - 1)]
                out[6 + k] = x[:, e & ~3]
            return out, None
        if fam == "votes":
            m = U(0) == 1
            ballot = (m.astype(np.uint64) << np.arange(64, dtype=np.uint64)).sum(axis=1, dtype=np.uint64)
            l = su(0).astype(np.int64)
            v = np.arange(nvec)
            return {0: m.any(axis=1).astype(np.uint32), 1: (ballot & np.uint64(0xFFFFFFFF)).astype(np.uint32),
                    2: (ballot >> np.uint64(32)).astype(np.uint32), 3: F(1)[v, l], 4: U(2)[v, l], 5: (F(1) + F(3))[v, l]}, None
        if fam == "lane_policy":
            t = mem.reshape(nvec, 128)
            m = (t[:, :64] & 1) != 0
            ballot = (m.astype(np.uint64) << np.arange(64, dtype=np.uint64)).sum(axis=1, dtype=np.uint64)
            omem[:, 0] = t[:, 0]
            return {0: (ballot & np.uint64(0xFFFFFFFF)).astype(np.uint32), 1: (ballot >> np.uint64(32)).astype(np.uint32),
                    2: t[:, 64:].view(np.int32).max(axis=1).astype(np.int32).view(np.uint32)}, omem
        if fam == "group_exchange":
            a, b, ua, m, X, every = F(0), F(1), U(2), U(3) == 1, F(4), U(5) == 1
            out = {0: shift_up(a, sf(0)), 1: shift_up(a, INF), 2: fmin_reduce(b), 3: ua.min(axis=1),
                   4: m.any(axis=1).astype(np.uint32), 5: m.sum(axis=1).astype(np.uint32)}
            out.update({6 + l: X[:, l] for l in range(4)})
            if W > 1:
                out.update({10: X[:, 0], 11: X[:, 1], 12: shift_up(a, sf(0)), 13: every.any(axis=1).astype(np.uint32)})
            return out, None
        if fam == "group_rec":
            mode = su(1)
            out = {}
            for k in range(3):
                last = F(k)[:, 63::64]  # what each wavefront's last lane published
                front = np.where(mode == 1, F(4 + k)[:, -1], INF)  # the carry, or +inf, in front of wavefront 0
                prev = np.concatenate([front[:, None], last[:, :-1]], axis=1)
                out[k] = np.repeat(prev, 64, axis=1)
            return out, None
        if fam in ("group_tdd", "group_tdd_strip"):
            E, could = inp["expect"]
            out = {0: E, 1: could.astype(np.uint32)}
            if fam == "group_tdd_strip":
                Q = targs[0]
                last = F(Q + 2)[:, 63::64]
                front = np.where(su(3) != 0, F(Q + 2)[:, -1], INF)
                out[2] = np.repeat(np.concatenate([front[:, None], last[:, :-1]], axis=1), 64, axis=1)
            return out, None
        if fam == "stash":
            Q = targs[0]
            out = {}
            for q in range(Q):
                out[q] = F(q) + F(Q)
                out[Q + q] = F(q)
                if W == 1:
                    out[2 * Q + q] = F(q) + F(Q)
            return out, None
        if fam == "pack_stash":
            Q = targs[0]
            add = F(6 * Q) if ctx == "valu" else None
            v = {(a, q): F(a * Q + q) + add if add is not None else F(a * Q + q) for a in range(6) for q in range(Q)}
            out = {a * Q + q: v[a, q] for a in range(6) for q in range(Q)}
            if ctx == "twice":
                out.update({6 * Q + a * Q + q: v[5 - a, q] for a in range(6) for q in range(Q)})
            return out, None
        if fam == "load_store_q":
            Q = targs[0]
            out = {q: memf[su(0)[:, None] + e * Q + q] for q in range(Q)}
            for v in range(nvec):
                for q in range(Q):
                    omem[v, su(1)[v] + e * Q + q] = vin[v, q]
            return out, omem
        if fam == "row_q":
            Q = targs[0]
            base = su(1)[:, None] // 4
            out = {0: memf[base[:, 0]], 1: memf[base[:, 0] + 1], 2: np.broadcast_to((16 + 4 * Q * e).astype(np.uint32), (nvec, 64))}
            out.update({3 + q: memf[base + ROW_HDR + e * Q + q] for q in range(Q)})
            return out, None
        if fam == "row_chunks":
            Q = targs[0]
            N = (Q + 3) // 4
            out = {}
            w, el = e // 64, e % 64
            for c in range(N):
                wc = min(4, Q - 4 * c)
                canon = 4 * ROW_HDR + 4 * Q * e + 16 * c
                order = 4 * COST_ORDER_HDR + 256 * Q * w + 1024 * c + 4 * wc * el
                off = np.where(su(2)[:, None] != 0, order, canon)
                out[c] = off.astype(np.uint32)
                for i in range(wc):
                    out[N + 4 * c + i] = memf[(su(1)[:, None] + off) // 4 + i]
            return out, None
        if fam == "pack_q":
            Q = targs[0]
            stride = scal[:, 0].astype(np.int64)[:, None] + ROW_HDR
            return {q: memf[U(1).astype(np.int64) * stride + U(0) // 4 + q] for q in range(Q)}, None
        if fam == "code_row":
            at, ncode = su(1)[:, None].astype(np.int64), su(2)[:, None]
            row = U(1).astype(np.int64)
            return {t: np.where(row < ncode, mem[at + np.minimum(row, ncode - 1) * 8 + t], 0).astype(np.uint32) for t in range(5)}, None
        if fam == "cols":
            return {q: memf[su(0)[:, None] + U(0) + q] for q in range(targs[0])}, None
        if fam == "lds":
            return {q: memf[U(0) + q] for q in range(targs[0])}, None
        if fam == "nodes":
            Q = targs[0]
            h = omem.view(np.uint16)
            for v in range(nvec):
                K = int(su(0)[v])
                for q in range(Q):
                    k = e * Q + q
                    h[v, k[k < K]] = vin[v, q][k < K].astype(np.uint16)
            return {}, omem
        if fam == "lane_mem":
            for v in range(nvec):
                omem[v, :64] = vin[v, 3]
                who = U(2)[v] == 1
                omem[v, 64 + U(1)[v][who]] = vin[v, 4][who]
                omem[v, 128:133] = vin[v, 5:10, 0]
                omem[v, 136] = scal[v, 0]
                omem[v, 137] = scal[v, 1]
            return {0: memf[U(0)], 1: memf[U(0)], 2: mem[U(0)]}, omem
    raise KeyError(name)


@pytest.mark.parametrize("name", names())
def test_emulator_against_numpy(em, name):
    W, nin, nout, _ = em.table()[name]
    inp = lc.case_inputs(name, W, nin, nout)
    out, omem = em.run(name, inp)
    want, want_omem = expected(name, W, inp)
    assert want or want_omem is not None
    for j, x in want.items():
        x = np.asarray(x)
        if x.ndim == 1:  # a uniform result: the same word in every lane
            x = np.broadcast_to(x[:, None], (x.shape[0], 64 * W))
        words = fbits(x.astype(f32)) if x.dtype.kind == "f" else np.ascontiguousarray(x).astype(np.uint32)
        ok = lc.same_words(out[:, j], words.reshape(out[:, j].shape))
        assert ok.all(), (name, j, np.argwhere(~ok)[:5], out[:, j][~ok][:5], words.reshape(ok.shape)[~ok][:5])
    if want_omem is not None:
        ok = lc.same_words(omem, want_omem)
        assert ok.all(), (name, "omem", np.argwhere(~ok)[:5])
    else:
        assert (omem == SENTINEL).all(), name  # a case without stores leaves its output memory alone
    assert em.lib.lane_conf_row_range_zeros() == 0, name  # every row read of these inputs lies inside its resource


def test_inputs_hold_what_the_ops_must_meet(em):
    """the edges the issue of this suite names are in the inputs, not left to chance"""
    t = em.table()
    a = ffrom(lc.case_inputs("wave_min/load", 1, 3, 2)["in"][:, 0])
    assert all((a[v].argmin() == v) for v in range(64))  # the minimum in each of the 64 lanes in turn
    assert any(np.isinf(r).all() for r in a)
    assert any((r != 0).all() and (np.abs(r) < 1.2e-38).all() for r in a)  # denormals only
    assert any((r == 0).all() and np.signbit(r).sum() == 1 for r in a)  # +0 with one -0
    ef = lc.case_inputs("elem_f", 1, 3, 12)["in"]
    x, y = ffrom(ef[:, 0]).ravel(), ffrom(ef[:, 1]).ravel()
    pz, nz = (x == 0) & ~np.signbit(x), (x == 0) & np.signbit(x)
    assert (pz & (y == 0) & np.signbit(y)).any() and (nz & (y == 0) & ~np.signbit(y)).any()  # +0/-0 in both orders
    assert (np.isnan(x) & np.isfinite(y)).any() and (np.isfinite(x) & np.isnan(y)).any()  # a NaN beside a number
    assert (np.isinf(x) & (x > 0) & np.isinf(y) & (y < 0)).any()
    g = ffrom(lc.case_inputs("groups<32>", 1, 2, 8)["in"][:, 0])
    assert all(g[v].argmin() == v for v in range(64))  # so in either DPP row of every group of 32
    for name in (n for n in t if n.startswith("group_tdd")):
        W, nin, nout, _ = t[name]
        inp = lc.case_inputs(name, W, nin, nout)
        E, could = inp["expect"]
        assert could.any() and (~could).any(), name  # on both sides of the threshold
        assert (E == f32(-996.25)).any() and (E >= 0).any(), name  # a negative E that cancels against tdd
        Q = nin - 4
        DD = ffrom(inp["in"][:, :Q])
        # mixed magnitude: adding a wavefront's DD lane after lane instead gives other bits
        differs = 0
        for v in range(DD.shape[0]):
            t64 = np.where(np.arange(64) == 0, f32(0), DD[v, 0, :64])
            for q in range(1, Q):
                t64 = (t64 + DD[v, q, :64]).astype(f32)
            serial = f32(0)
            for x64 in t64:
                serial = f32(serial + x64)
            differs += fbits(serial) != fbits(lc.wave_tdd(DD[v][:, :64]))
        assert differs >= DD.shape[0] // 2, (name, differs)
    cr = lc.case_inputs("code_row", 1, 2, 5)
    rows, ncode = cr["in"][:, 1], cr["scal"][0, 2]
    assert {ncode - 1, ncode, ncode + 5} <= set(rows.ravel().tolist())
    for Q in (5, 10):
        rc = lc.case_inputs(f"row_chunks<{Q},2>", 2, 0, 0)
        s = rc["scal"]
        assert (s[:, 1] != 0).any() and ((s[:, 1] + s[:, 0] // 3) == s[:, 0]).any()  # a row offset; the resource's last row
        assert set(s[:, 2].tolist()) == {0, 1}  # both layouts
