"""CPU: the memory plan of the path pass (deciphon_amd/csrc/path_plan.h, through dcp_path_plan_of): which strip
windows go in blocks, how many blocks G go side by side, and what every window places -- against the layout restated in
tests/path_layout.py and the rules restated below, neither of which calls the planner."""
import pytest

from deciphon_amd import host
from deciphon_amd.hip import HipError
from path_layout import (MB, WAVES, aligned, block_table_bytes_of, ckpt_bytes_of, group_tables_bytes_of, num_blocks,
                         padded, scratch_bytes, table_bytes, table_bytes_of)

FAST, LITERAL = host.PATH_FAST, host.PATH_LITERAL


def strip(L, K):
    return (L, K, padded(K), WAVES, 1)


def short(L, K, Kp, W):
    return (L, K, Kp, W, 0)


# ---- the rules, as csrc/path_plan.h states them ----
def whole_bytes(kind, w):
    """what a strip window takes when it keeps its whole table: the test of the strip decision"""
    L, K, Kp = w[:3]
    return table_bytes_of(L, Kp) if kind == FAST else aligned(table_bytes_of(L, Kp)) + scratch_bytes(L + 1, K)


def in_blocks(kind, w, B, budget, strict):
    return not (w[4] or kind == LITERAL) or (B > 0 and whole_bytes(kind, w) > budget and not strict)


def per_block(kind, w, B):
    L, K, Kp = w[:3]
    return block_table_bytes_of(L, Kp, B) + (scratch_bytes(B + 6, K) if kind == LITERAL else 0)


def ckpts(kind, w, B):
    L, K, Kp, W, s = w
    return ckpt_bytes_of(L, Kp, W, B, bool(s) or kind == LITERAL)


def group_size(kind, wins, B, budget, strict=False, chunk=0, override=0):
    inb = [w for w in wins if in_blocks(kind, w, B, budget, strict)]
    fold = sum if kind == FAST else (lambda v: max(v, default=0))
    one = fold([per_block(kind, w, B) for w in inb])
    fixed = fold([ckpts(kind, w, B) for w in inb])
    if kind == FAST:
        fixed += sum(table_bytes_of(w[0], w[2]) for w in wins if w not in inb)
    most = max([num_blocks(w[0], B) for w in inb], default=1)
    cap = 1 << 31
    for w in inb:
        if chunk:
            room = chunk - ckpts(kind, w, B) - 1024
            cap = min(cap, room // per_block(kind, w, B) if room > per_block(kind, w, B) else 1)
    room = 0.9 * budget - fixed
    G = min(int(min(room / one, most)) if one > 0 and room > one else 1, cap)
    if override > 0:
        G = override
    return max(1, min(G, most))


def placement(kind, w, B, budget, strict, G):
    """-> (in_blocks, blocks, replay_rows, ckpt_off, scratch_off, bytes) of one window"""
    L, K, Kp = w[:3]
    inb = in_blocks(kind, w, B, budget, strict)
    if not inb:
        nb, ckpt_off, tables, rows = 1, 0, table_bytes_of(L, Kp), L + 1
    else:
        nb, ckpt_off = num_blocks(L, B), group_tables_bytes_of(L, Kp, B, G)
        tables, rows = ckpt_off + ckpts(kind, w, B), min(G, nb) * (B + 6)
    if kind == FAST:
        return (inb, nb, 0, ckpt_off, 0, tables)
    return (inb, nb, rows, ckpt_off, aligned(tables), aligned(tables) + scratch_bytes(rows, K))


def check(kind, wins, B, budget, strict=False, chunk=0, override=0):
    """the plan of the library, held against the rules and against its own bounds"""
    wins = [w for w in wins if w[4]] if kind == LITERAL else wins
    plan = host.path_plan(kind, wins, B, budget, strict, chunk, override)
    G = group_size(kind, wins, B, budget, strict, chunk, override)
    assert plan["G"] == G
    assert plan["blocked"] == sum(1 for w in wins if (w[4] or kind == LITERAL) and in_blocks(kind, w, B, budget, strict))
    for i, w in enumerate(wins):
        got = tuple(int(plan[k][i]) for k in ("in_blocks", "blocks", "replay_rows", "ckpt_off", "scratch_off", "bytes"))
        assert got == tuple(int(v) for v in placement(kind, w, B, budget, strict, G)), (kind, B, w)
        inb, nb, rows, ckpt_off, scratch_off, nbytes = got
        L, K, Kp = w[:3]
        if inb:  # min(G, blocks) tables, then the checkpoints, inside the placement
            tables = min(G, nb) * block_table_bytes_of(L, Kp, B)
            assert tables <= ckpt_off < tables + 16
            assert ckpt_off + ckpts(kind, w, B) <= nbytes
        else:
            assert ckpt_off == 0 and nb == 1 and table_bytes_of(L, Kp) <= nbytes
        if kind == LITERAL:
            assert scratch_off % 256 == 0 and scratch_off >= ckpt_off + (ckpts(kind, w, B) if inb else 0)
            assert scratch_off + rows * 3 * K * 4 <= nbytes
    return plan


MIX = [strip(120, 4200), short(120, 300, 384, 1), strip(3000, 4200), strip(600, 8192), short(2000, 1000, 1024, 4)]
BUDGET = 64 * MB  # holds the whole table of the first and (fast pass only) the fourth window, not of the third


@pytest.mark.parametrize("B", [0, 5, 50, 500])
@pytest.mark.parametrize("kind", [FAST, LITERAL])
def test_every_placement_is_the_layouts(kind, B):
    for override in (0, 1, 2, 7):
        plan = check(kind, MIX, B, BUDGET, override=override)
        if B > 0:  # (3000, 4200) in both; (600, 8192) too once its scratch comes on top
            assert plan["blocked"] == (1 if kind == FAST else 2)
        else:
            assert plan["blocked"] == 0 and plan["G"] == 1


@pytest.mark.parametrize("B", [5, 50, 500])
@pytest.mark.parametrize("kind", [FAST, LITERAL])
def test_block_count_edges(kind, B):
    """L = B + 5 is the last window of one block, B + 6 has two, 2 B + 6 is the first with three; a G beyond a window's
    blocks places only that many tables"""
    K = 4200
    lengths = [B + 5, B + 6, 2 * B + 5, 2 * B + 6]
    assert [num_blocks(L, B) for L in lengths] == [1, 2, 2, 3]
    for G in (1, 2, 3, 5):
        wins = [strip(L, K) for L in lengths] + [short(L, 300, 384, 1) for L in lengths]
        plan = check(kind, wins, B, 1, override=G)  # a budget of one byte: every strip window in blocks
        n = len(lengths)
        assert list(plan["blocks"][:n]) == [1, 2, 2, 3] and plan["G"] == min(G, 3)
        for i, L in enumerate(lengths):
            assert plan["ckpt_off"][i] == aligned(min(G, num_blocks(L, B)) * block_table_bytes_of(L, padded(K), B), 16)
            if kind == LITERAL:
                assert plan["replay_rows"][i] == min(G, 3, num_blocks(L, B)) * (B + 6)


@pytest.mark.parametrize("kind", [FAST, LITERAL])
def test_the_strip_decision_at_the_budget(kind):
    """the whole table is kept up to the budget and given up one byte below: of the table alone in the fast plan, of the
    table rounded up to 256 and the scratch of all its rows in the literal plan"""
    w, B = strip(600, 4200), 50
    at = whole_bytes(kind, w)
    assert whole_bytes(FAST, w) == table_bytes(600, 4200) < whole_bytes(LITERAL, w)
    fits = check(kind, [w], B, at)
    assert fits["blocked"] == 0 and not fits["in_blocks"][0] and fits["ckpt_off"][0] == 0
    over = check(kind, [w], B, at - 1)
    assert over["blocked"] == 1 and over["in_blocks"][0] and over["blocks"][0] == num_blocks(600, B) == 12
    strict = check(kind, [w], B, at - 1, strict=True)
    assert strict["blocked"] == 0 and not strict["in_blocks"][0] and strict["bytes"][0] == fits["bytes"][0]
    assert check(kind, [w], 0, 1)["blocked"] == 0  # no checkpoints, no blocks
    # between the two thresholds the passes differ
    assert check(FAST, [w], B, whole_bytes(FAST, w))["blocked"] == 0
    assert check(LITERAL, [w], B, whole_bytes(FAST, w))["blocked"] == 1


def test_the_fast_plan_sums_and_the_literal_plan_takes_the_most():
    """two windows in blocks under 150 MB: their block tables side by side (75 MB a round) leave the fast plan one
    block at a time, while the literal plan, which sizes G for one window (63 MB with its scratch), takes two"""
    wins, B, budget = [strip(3000, 4200), strip(3000, 4200)], 500, 150 * MB
    fast = check(FAST, wins, B, budget)
    literal = check(LITERAL, wins, B, budget)
    assert fast["blocked"] == literal["blocked"] == 2
    assert (fast["G"], literal["G"]) == (1, 2)


def test_the_chunk_cap_and_the_override():
    w, B, budget = strip(3000, 4200), 500, 200 * MB
    assert num_blocks(3000, B) == 6
    for kind, free in ((FAST, 5), (LITERAL, 2)):  # what 90 % of the budget holds, nothing else in the way
        one, fixed = per_block(kind, w, B), ckpts(kind, w, B)
        assert check(kind, [w], B, budget, chunk=0)["G"] == free
        assert check(kind, [w], B, budget, chunk=fixed + 1024 + 2 * one)["G"] == 2 == min(free, 2)
        assert check(kind, [w], B, budget, chunk=fixed + 1024 + one + 1)["G"] == 1
        assert check(kind, [w], B, budget, chunk=fixed + 1024 + one)["G"] == 1
        assert check(kind, [w], B, budget, chunk=fixed + 1024 + one + 1, override=5)["G"] == 5  # wins over the cap
        assert check(kind, [w], B, budget, chunk=fixed + 1024 + one + 1, override=100)["G"] == 6  # but not over `most`
        assert check(kind, [w], B, budget, override=1)["G"] == 1


def test_a_plan_stays_within_the_budget_its_windows_fit():
    """G leaves a tenth of the budget free -- G * one + fixed <= 0.9 budget whenever G > 1 -- and the alignments of a
    placement are below 1 KB a window: where every window fits the budget one block at a time, every placement of the
    plan does, and a fast plan with G > 1 fits it as a whole (one slice: the sum rule)."""
    held = 0
    for wins, B, budget in ((MIX, 500, BUDGET), (MIX, 50, BUDGET), (MIX, 5, BUDGET), (MIX, 500, 300 * MB),
                            ([strip(3000, 4200)] * 2, 500, 150 * MB), ([strip(3000, 4200)] * 2, 500, 200 * MB),
                            ([strip(3000, 4200)] * 3, 500, 200 * MB), ([strip(3000, 4200)] * 3, 50, 200 * MB),
                            ([short(2000, 1000, 1024, 4)] * 40, 500, 600 * MB)):
        for kind in (FAST, LITERAL):
            ws = [w for w in wins if w[4]] if kind == LITERAL else wins
            if not all(aligned(placement(kind, w, B, budget, False, 1)[5]) <= budget for w in ws):
                continue
            plan = check(kind, ws, B, budget)
            assert all(aligned(int(b)) <= budget for b in plan["bytes"])
            if kind == FAST and plan["G"] > 1:
                assert sum(aligned(int(b)) for b in plan["bytes"]) <= budget
                held += 1
    assert held >= 3


def test_bad_arguments_are_refused():
    for bad in (dict(kind=2), dict(B=-5), dict(budget=-1)):
        a = dict(kind=FAST, windows=[strip(120, 4200)], B=50, budget=MB)
        a.update(bad)
        with pytest.raises(HipError):
            host.path_plan(**a)
    assert host.path_plan(FAST, [], 50, MB)["G"] == 1
