"""CPU: the plan of a window list (deciphon_amd/csrc/stage_plan.h, through dcp_stage_plan_of and dcp_cost_schedule_of)
-- refusals, problems, packs, LDS groups, both orderings, the shares of the lists, the trellis arena, and the launches of
a cost pass -- against the model below, which sorts with sorted() and cuts greedily and calls none of it.  The profiles
are described by the engine's own tables (dcp_engine_core_size, dcp_engine_pack_shape)."""
import functools

import numpy as np
import pytest

from deciphon_amd import host
from deciphon_amd.hip import HipError

NC, NS = host.NUM_CLASSES, host.NUM_PACK_SHAPES
NONE, TRELLIS, TABLE = host.ARENA_NONE, host.ARENA_TRELLIS, host.ARENA_TABLE
# every boundary of a class, a narrow limit and a pack shape
KS = (3, 4, 12, 13, 60, 61, 64, 65, 124, 125, 256, 257, 320, 321, 448, 449, 640, 641, 768, 4096, 4097)
READS = (30, 31, 45, 90, 120, 200, 333, 1)


@functools.lru_cache(None)
def describe(K):
    return host.engine_core_size(K)  # (K, Kp, class, narrow, pack shape)


@functools.lru_cache(None)
def shapes():
    return tuple(tuple(int(v) for v in row) for row in host.engine_pack_shapes())  # (windows, lds waves) per shape


def offsets(reads):
    so = np.concatenate([[0], np.cumsum(reads)]).astype(np.int64)
    return so, so + np.arange(len(so))  # a read of n nucleotides has n + 1 code rows


def align16(n):
    return (n + 15) & ~15


# ---- the model ----
def model(wins, prof, row_off, arena=NONE, table_addr=None, pack=True, lds=True):
    P, at = [], 0
    for i, (p, s, a, b) in enumerate(wins):
        K, Kp = prof[p][:2]
        L = b - a
        size = (L + 1) * 4 + (L + 1) * K * 2 if arena == TRELLIS else (L + 1) * (8 + 3 * Kp) * 4
        trellis = 0 if arena == NONE else at if arena == TRELLIS else int(table_addr[i])
        at += align16(size) if arena != NONE else 0
        P.append(dict(profile=p, L=L, code_row=int(row_off[s]) + a, xt_row=max(L // 3, 1), out=i, trellis=trellis))
    packing = pack and arena == NONE and int(row_off[-1]) < 2 ** 32
    shape = lambda q: prof[q["profile"]][4] if packing else -1
    packed = sorted((q for q in P if shape(q) >= 0), key=lambda q: (shape(q), q["profile"], -q["L"]))
    rest = sorted((q for q in P if shape(q) < 0), key=lambda q: (prof[q["profile"]][2], not prof[q["profile"]][3], q["profile"]))
    packs = []  # lists of problems
    for q in packed:
        if not packs or packs[-1][0]["profile"] != q["profile"] or len(packs[-1]) == shapes()[shape(q)][0]:
            packs.append([])
        packs[-1].append(q)
    groups, pk_begin, pg_begin = [], [0] * (NS + 1), [0] * (NS + 1)
    for s in range(NS):
        mine = [k for k in packs if shape(k[0]) == s]
        pk_begin[s + 1] = pk_begin[s] + len(mine)
        cut = []  # [first, count]
        for j, k in enumerate(mine):
            if not lds or not shapes()[s][1]:
                break
            if not cut or mine[cut[-1][0]][0]["profile"] != k[0]["profile"] or cut[-1][1] == shapes()[s][1]:
                cut.append([j, 0])
            cut[-1][1] += 1
        groups += cut
        pg_begin[s + 1] = len(groups)
    cls = [prof[q["profile"]][2] for q in rest]
    narrow = [bool(prof[q["profile"]][3]) for q in rest]
    c_begin = [sum(c < k for c in cls) for k in range(NC + 1)]
    c_wide = [c_begin[k] + sum(c == k and n for c, n in zip(cls, narrow)) for k in range(NC)]
    c_profiles = [[len({q["profile"] for q, c, n in zip(rest, cls, narrow) if c == k and n == want}) for want in (True, False)]
                  for k in range(NC)]
    return dict(problems=rest, packs=packs, groups=groups, c_begin=c_begin, c_wide=c_wide, c_profiles=c_profiles,
                pk_begin=pk_begin, pg_begin=pg_begin, cells=float(sum(prof[p][0] * (b - a) for p, _, a, b in wins)),
                arena_bytes=at, max_xt_row=max([q["xt_row"] for q in P] + [1]))


def check(wins, prof, reads, row_off=None, **kw):
    """the plan of these windows against the model, element for element; returns the plan"""
    so, ro = offsets(reads)
    ro = ro if row_off is None else np.asarray(row_off, np.int64)
    got = host.stage_plan(wins, prof, so, ro, arena=kw.get("arena", NONE), table_addr=kw.get("table_addr"),
                          pack=kw.get("pack", True), pack_lds=kw.get("lds", True))
    want = model([tuple(int(v) for v in w) for w in wins], prof, ro, **kw)
    assert len(got["problems"]) == len(want["problems"])
    for f in ("profile", "L", "code_row", "xt_row", "out", "trellis"):
        assert got["problems"][f].tolist() == [q[f] for q in want["problems"]], f
    assert len(got["packs"]) == len(want["packs"])
    for pk, k in zip(got["packs"], want["packs"]):
        assert pk["profile"] == k[0]["profile"] and pk["Lmax"] == k[0]["L"] == max(q["L"] for q in k)
        for f in ("L", "xt_row", "out", "code_row"):  # idle groups: L = 0, and everything else
            assert pk[f].tolist() == [q[f] for q in k] + [0] * (16 - len(k)), f
    assert got["groups"].tolist() == want["groups"]
    for f in ("c_begin", "c_wide", "c_profiles", "pk_begin", "pg_begin"):
        assert got[f].tolist() == want[f], f
    assert got["cells"] == want["cells"] and got["arena_bytes"] == want["arena_bytes"]
    assert got["max_xt_row"] == want["max_xt_row"]
    return got


def all_windows(nprof, reads):
    """ascending by profile: whole reads, and a window inside every read that has room"""
    wins = []
    for p in range(nprof):
        for s, n in enumerate(reads):
            wins.append((p, s, 0, n))
            if n > 40:
                wins.append((p, s, 7, 7 + 30 + (p + s) % 9))
    return wins


# ---- orderings ----
@pytest.mark.parametrize("lds", [True, False])
def test_the_two_orderings_agree_with_the_model(lds):
    """Ascending by profile: the counting path; the same windows shuffled: the comparison path."""
    prof = [describe(K) for K in KS]
    wins = all_windows(len(prof), READS)
    assert all(a[0] <= b[0] for a, b in zip(wins, wins[1:]))
    sorted_plan = check(wins, prof, READS, lds=lds)
    assert len(sorted_plan["packs"]) > NS and (len(sorted_plan["groups"]) > 0) == lds
    rng = np.random.default_rng(5)
    for _ in range(3):
        order = rng.permutation(len(wins))
        assert any(wins[a][0] > wins[b][0] for a, b in zip(order, order[1:]))
        shuffled = check([wins[i] for i in order], prof, READS, lds=lds)
        for f in ("c_begin", "c_wide", "c_profiles", "pk_begin", "pg_begin"):  # the same shares, whatever the order
            assert shuffled[f].tolist() == sorted_plan[f].tolist(), f


@pytest.mark.parametrize("order", ["longest first", "ascending", "mixed"])
@pytest.mark.parametrize("distinct", [1, 2, 32, 33, 40])
def test_longest_first_in_every_regime(distinct, order):
    """One profile's run of windows with 1 .. 40 distinct lengths (32 is the most the counting pass takes), every length
    twice and once more for some: equal lengths keep their input order (the model's sorted() is stable, and `out` tells)."""
    prof = [describe(12), describe(13)]
    lengths = [50 + 3 * i for i in range(distinct)]
    run = [L for L in lengths for _ in range(2 + L % 2)]
    if order == "longest first":
        run.sort(reverse=True)
    elif order == "ascending":
        run.sort()
    else:
        run = [run[i] for i in np.random.default_rng(distinct).permutation(len(run))]
    wins = [(0, 0, i % 5, i % 5 + L) for i, L in enumerate(run)] + [(1, 0, 0, L) for L in run[:5]]
    plan = check(wins, prof, (400,))
    mine = [(int(L), int(o)) for pk in plan["packs"] if pk["profile"] == 0 for L, o in zip(pk["L"], pk["out"]) if L]
    assert mine == sorted(mine, key=lambda t: (-t[0], t[1])) and len(mine) == len(run)


# ---- packs, groups and counts ----
@pytest.mark.parametrize("K", [3, 12, 60, 124])
@pytest.mark.parametrize("extra", [-1, 0, 1])
def test_packs_around_a_full_pack(K, extra):
    prof = [describe(K), describe(K)]
    G = shapes()[prof[0][4]][0]
    n = G + extra
    reads = tuple(20 + 3 * i for i in range(n))
    wins = [(p, s, 0, reads[s]) for p in range(2) for s in range(n)]
    plan = check(wins, prof, reads)
    packs = plan["packs"]
    assert len(plan["problems"]) == 0 and len(packs) == 2 * (1 if n <= G else 2)
    for pk in packs:
        live = pk["L"][pk["L"] > 0]
        assert pk["Lmax"] == pk["L"][0] == live.max() and 1 <= len(live) <= G
        assert {wins[o][0] for o in pk["out"][: len(live)]} == {int(pk["profile"])}  # never two profiles in a pack
    pk_begin = plan["pk_begin"].tolist()
    assert pk_begin == sorted(pk_begin) and pk_begin[-1] == len(packs) and pk_begin[0] == 0


def test_groups_count_from_their_shapes_first_pack():
    prof = [describe(K) for K in KS]
    wins = [w for w in all_windows(len(prof), READS) for _ in range(5)]  # enough packs per profile for several groups
    plan = check(wins, prof, READS)
    pk, pg = plan["pk_begin"], plan["pg_begin"]
    assert pg[-1] == len(plan["groups"]) > 0 and pg.tolist() == sorted(pg.tolist())
    for s in range(NS):
        windows, waves = shapes()[s]
        mine = plan["groups"][pg[s] : pg[s + 1]]
        assert (waves == 0) == (windows == 2)  # groups of 32 lanes: no LDS variant
        if waves == 0 or pk[s + 1] == pk[s]:  # (no core size of KS lands in shapes 4, 5 and 6)
            assert len(mine) == 0
            continue
        assert len(mine) > 0 and mine[0][0] == 0 and mine[:, 1].max() <= waves and mine[:, 1].min() >= 1
        assert mine[:, 1].sum() == pk[s + 1] - pk[s]  # every pack of the shape in exactly one group, in order
        assert (mine[1:, 0] == np.cumsum(mine[:-1, 1])).all()
        for first, count in mine:
            assert len({int(p) for p in plan["packs"]["profile"][pk[s] + first : pk[s] + first + count]}) == 1
    off = check(wins, prof, READS, lds=False)
    assert len(off["groups"]) == 0 and not off["pg_begin"].any()
    assert off["packs"].tobytes() == plan["packs"].tobytes()


def test_every_out_slot_once_and_the_cells():
    prof = [describe(K) for K in KS]
    wins = all_windows(len(prof), READS)
    order = np.random.default_rng(3).permutation(len(wins))
    for ws in (wins, [wins[i] for i in order]):
        plan = check(ws, prof, READS)
        outs = plan["problems"]["out"].tolist() + [int(o) for pk in plan["packs"] for o, L in zip(pk["out"], pk["L"]) if L]
        assert sorted(outs) == list(range(len(ws)))
        assert plan["cells"] == float(sum(prof[p][0] * (b - a) for p, _, a, b in ws))


def test_narrow_and_wide_shares_of_a_class():
    """class 4 holds K = 300 (narrow: up to 320) and 350; class 5 only narrow profiles here, class 6 only wide ones"""
    Ks = (300, 350, 310, 400, 440, 700, 650)
    prof = [describe(K) for K in Ks]
    assert [(p[2], p[3]) for p in prof] == [(4, 1), (4, 0), (4, 1), (5, 1), (5, 1), (6, 0), (6, 0)]
    wins = [(p, s, 0, READS[s]) for p in range(len(Ks)) for s in range(p + 1)]  # p + 1 windows of profile p
    for ws in (wins, wins[::-1]):
        plan = check(ws, prof, READS)
        assert plan["c_begin"][4:8].tolist() == [0, 6, 15, 28]
        assert plan["c_wide"][4:7].tolist() == [4, 15, 15]  # 1 + 3 narrow windows; all nine; none
        assert plan["c_profiles"][4:7].tolist() == [[2, 1], [2, 0], [0, 2]]
        assert not plan["c_profiles"][:4].any() and not plan["c_profiles"][7:].any()


# ---- switches and limits ----
def test_when_packing_is_off():
    prof = [describe(K) for K in (3, 60, 300)]
    reads = (50, 60)
    wins = [(p, 0, 0, 40 + p) for p in range(3) for _ in range(3)]  # read 0 only: the code rows used stay small
    assert len(check(wins, prof, reads)["packs"]) == 2
    assert len(check(wins, prof, reads, pack=False)["packs"]) == 0
    assert len(check(wins, prof, reads, arena=TRELLIS)["packs"]) == 0
    assert len(check(wins, prof, reads, arena=TABLE, table_addr=[4096 * i for i in range(9)])["packs"]) == 0
    # code rows are addressed by u32 index in a pack: 2^32 of them in all is one too many (synthetic offsets: nothing
    # is allocated by them)
    most = check(wins, prof, reads, row_off=[0, 51, 2 ** 32 - 1])
    assert len(most["packs"]) == 2 and len(most["problems"]) == 3
    beyond = check(wins, prof, reads, row_off=[0, 51, 2 ** 32])
    assert len(beyond["packs"]) == 0 and len(beyond["problems"]) == 9 and not beyond["pk_begin"].any()


# ---- arena ----
def test_trellis_arena_in_the_order_given():
    prof = [describe(K) for K in (3, 173, 300, 4097)]
    wins = [(3, 4, 0, 120), (0, 0, 0, 30), (2, 3, 5, 90), (1, 2, 0, 45), (0, 1, 1, 30), (3, 5, 0, 200)]
    plan = check(wins, prof, READS, arena=TRELLIS)
    L, K = [b - a for _, _, a, b in wins], [prof[p][0] for p, _, _, _ in wins]
    off, total = host.trellis_arena(L, K)  # what the literal path pass lays out before it stages
    sizes = [align16((l + 1) * 4 + (l + 1) * k * 2) for l, k in zip(L, K)]
    assert off.tolist() == [sum(sizes[:i]) for i in range(len(wins))] and total == sum(sizes) == plan["arena_bytes"]
    assert plan["problems"]["trellis"][np.argsort(plan["problems"]["out"])].tolist() == off.tolist()


def test_table_arena_takes_the_addresses_given():
    prof = [describe(K) for K in (3, 173, 300)]
    wins = [(2, 3, 5, 90), (0, 0, 0, 30), (1, 2, 0, 45), (0, 1, 1, 30)]
    addr = [0x7F0000001000, 0x7F0000900000, 0x7F0000100000, 0x7E0000000100]
    plan = check(wins, prof, READS, arena=TABLE, table_addr=addr)
    assert plan["problems"]["trellis"][np.argsort(plan["problems"]["out"])].tolist() == addr


# ---- refusals ----
GOOD = (0, 0, 0, 30)
BAD = {"bad profile index": [(-1, 0, 0, 30), (2, 0, 0, 30)], "bad sequence index": [(0, -1, 0, 30), (0, 8, 0, 30)],
       "bad window range": [(0, 0, -1, 30), (0, 0, 20, 10), (0, 0, 0, 31), (0, 0, 40, 40)], "empty window": [(0, 0, 7, 7), (1, 1, 0, 0)]}


def refused(wins, prof=None, **kw):
    so, ro = offsets(READS)
    with pytest.raises(HipError) as e:
        host.stage_plan(wins, prof or [describe(12), describe(300)], so, ro, **kw)
    return e.value.code, str(e.value)


@pytest.mark.parametrize("what", list(BAD))
def test_each_window_check_alone(what):
    code = 11 if what == "empty window" else 8  # DCP_EZEROSEQ, DCP_EFUNCUSE
    for w in BAD[what]:
        for wins in ([w], [GOOD, w, GOOD]):
            got = refused(wins)
            assert got[0] == code and f"({what})" in got[1], (w, got)


def test_the_first_offending_window_and_its_first_failing_check():
    order = list(BAD)
    for i, a in enumerate(order):
        for b in order:
            if a != b:  # two bad windows: the first in list order, whichever check comes first
                assert f"({a})" in refused([GOOD, BAD[a][0], BAD[b][0]])[1]
        for b in order[i + 1 :]:  # one window bad in two ways: the earlier check
            both = {("bad profile index", "bad sequence index"): (9, 9, 0, 30), ("bad profile index", "bad window range"): (9, 0, 0, 99),
                    ("bad profile index", "empty window"): (9, 0, 3, 3), ("bad sequence index", "bad window range"): (0, 9, 5, 2),
                    ("bad sequence index", "empty window"): (0, 9, 3, 3), ("bad window range", "empty window"): (0, 0, 31, 31)}[(a, b)]
            assert f"({a})" in refused([GOOD, both])[1], (a, b)


def test_no_windows_and_a_profile_outside_every_class():
    so, ro = offsets(READS)
    plan = host.stage_plan(np.zeros((0, 4), np.int32), [describe(12)], so, ro)
    assert len(plan["problems"]) == len(plan["packs"]) == len(plan["groups"]) == 0 and plan["cells"] == 0
    assert not any(plan[f].any() for f in ("c_begin", "c_wide", "c_profiles", "pk_begin", "pg_begin"))
    for ws in ([GOOD, (1, 0, 0, 30)], [(1, 0, 0, 30), GOOD]):  # ascending and not: either ordering would index by class
        got = refused(ws, prof=[describe(12), (20000, 20480, -1, 0, -1)])
        assert got[0] == 63 and "(profile outside every kernel class)" in got[1]  # DCP_ELARGECORESIZE
    assert refused([GOOD, (1, 0, 0, 99)], prof=[describe(12), (20000, 20480, -1, 0, -1)])[0] == 8  # a window check goes first


# ---- the launches of a cost pass ----
def ranges(classes=None, packs=None):
    """classes: {class: (narrow windows, narrow profiles, wide windows, wide profiles)}; packs: {shape: (packs, groups)}"""
    r = dict(c_begin=[0] * (NC + 1), c_wide=[0] * NC, c_profiles=[[0, 0] for _ in range(NC)], pk_begin=[0] * (NS + 1),
             pg_begin=[0] * (NS + 1))
    for c in range(NC):
        nn, pn, nw, pw = (classes or {}).get(c, (0, 0, 0, 0))
        r["c_wide"][c] = r["c_begin"][c] + nn
        r["c_begin"][c + 1] = r["c_wide"][c] + nw
        r["c_profiles"][c] = [pn, pw]
    for s in range(NS):
        np_, ng = (packs or {}).get(s, (0, 0))
        r["pk_begin"][s + 1], r["pg_begin"][s + 1] = r["pk_begin"][s] + np_, r["pg_begin"][s] + ng
    return r


def launch(kernel, index, first, count, wpp=0, branch=None):
    return dict(kernel=kernel, index=index, first=first, count=count, windows_per_profile=wpp,
                branch=branch or {"narrow": "narrow", "pack": "pack", "pack_lds": "pack"}.get(kernel, "class"))


def test_schedule_of_one_class_alone():
    assert host.cost_schedule(ranges({7: (0, 0, 10, 3)})) == [launch("class", 7, 0, 10, 10 // 3)]  # one entry: no fork
    assert host.cost_schedule(ranges()) == []


def test_schedule_fuses_small_mixes_of_single_wave_classes():
    small = ranges({1: (0, 0, 8000, 3), 2: (0, 0, 8384, 7), 5: (0, 0, 50, 2)})
    assert host.cost_schedule(small) == [launch("class", 5, 16384, 50, 25), launch("fused", 0, 0, 16384)]
    large = ranges({1: (0, 0, 8000, 3), 2: (0, 0, 8385, 7), 5: (0, 0, 50, 2)})
    assert host.cost_schedule(large) == [launch("class", 5, 16385, 50, 25), launch("class", 2, 8000, 8385, 8385 // 7),
                                         launch("class", 1, 0, 8000, 8000 // 3)]
    assert host.cost_schedule(ranges({3: (0, 0, 100, 4)})) == [launch("class", 3, 0, 100, 25)]  # one class: nothing to fuse


def test_schedule_of_a_class_with_a_narrow_kernel():
    only_narrow = ranges({2: (0, 0, 5, 1), 4: (6, 2, 0, 0)})
    assert host.cost_schedule(only_narrow) == [launch("narrow", 4, 5, 6, 3), launch("none", 4, 11, 0), launch("class", 2, 0, 5, 5)]
    only_wide = ranges({2: (0, 0, 5, 1), 4: (0, 0, 9, 2)})
    assert host.cost_schedule(only_wide) == [launch("class", 4, 5, 9, 4), launch("class", 2, 0, 5, 5)]
    both = ranges({2: (0, 0, 5, 1), 4: (6, 2, 9, 2)})
    assert host.cost_schedule(both) == [launch("narrow", 4, 5, 6, 3), launch("class", 4, 11, 9, 4), launch("class", 2, 0, 5, 5)]


def test_schedule_with_the_narrow_kernels_switched_off():
    both = ranges({4: (6, 2, 9, 2), 6: (7, 1, 0, 0)})
    assert host.cost_schedule(both, narrow=False) == [launch("class", 6, 15, 7, 7), launch("class", 4, 0, 15, 15 // 4)]


def test_schedule_of_packs_with_and_without_groups():
    r = ranges({9: (0, 0, 4, 4)}, {0: (5, 2), 3: (7, 0), 10: (3, 0)})
    assert host.cost_schedule(r) == [launch("class", 9, 0, 4, 1), launch("pack", 10, 12, 3), launch("pack", 3, 5, 7),
                                     launch("pack_lds", 0, 0, 2)]
    r = ranges(None, {0: (5, 2), 1: (6, 3)})
    assert host.cost_schedule(r) == [launch("pack_lds", 1, 2, 3), launch("pack_lds", 0, 0, 2)]


def test_schedule_of_a_planned_list_covers_it():
    prof = [describe(K) for K in KS]
    plan = check(all_windows(len(prof), READS), prof, READS)
    for narrow in (True, False):
        s = host.cost_schedule(plan, narrow)
        problems = sorted((e["first"], e["count"]) for e in s if e["kernel"] in ("class", "narrow", "fused"))
        assert [f for f, _ in problems] == [0] + list(np.cumsum([c for _, c in problems])[:-1])
        assert sum(c for _, c in problems) == len(plan["problems"])
        assert sum(e["count"] for e in s if e["kernel"] == "pack_lds") == len(plan["groups"])
        assert [e["index"] for e in s if e["branch"] == "class"] == sorted((e["index"] for e in s if e["branch"] == "class"), reverse=True)
