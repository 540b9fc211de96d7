"""CPU: the window walk of dcp_scan_run (csrc/scan_walk.h, through include/deciphon_host.h dcp_scan_walk_*) against the
reference's own order of work -- for each profile, for each read, one window after the other, last_hit_pos set after
each hit (c-core/thread.c:162; host.WindowIter is pinned to c-core/window.c by tests/test_reference_unzip.py).  The
cost and path passes are played by a pure function of the window, so whatever the order in which the walk is driven --
one chunk, many chunks with two outstanding, path batches between chunks, nothing speculated -- it must find exactly
the reference's hits and walk exactly its windows."""
import collections
import struct
import zlib

import numpy as np
import pytest

from deciphon_amd import host

CORE_SIZES = [3, 12, 30, 60, 173]
# an empty read, reads shorter than one window, two of one length next to each other, one length that comes back
# after another (the per-profile chain cache)
READ_LENGTHS = [0, 1, 50, 1500, 9990, 10000, 30000, 30000, 120000, 1500]
BELOW, PASS, HIT = 0, 1, 2
FIRST_CELLS, PAIRS, CAP = 1.0e10, 1 << 21, 4 << 20  # what dcp_scan_run plans with by default


def score(profile, read, start, stop):
    """(outcome, lrt, last_hit_pos) of a window: 2 in 8 hit somewhere in the window, 1 in 8 pass the filter with a
    path that holds no hit, 5 in 8 stay below the filter."""
    crc = zlib.crc32(struct.pack("<4i", profile, read, start, stop))
    outcome = (HIT, HIT, PASS)[crc & 7] if crc & 7 < 3 else BELOW
    return outcome, np.float32(((crc >> 3) & 0xFFF) / 8.0), (crc >> 15) % (stop - start)


def chain(seq_size, core_size):
    it, out = host.WindowIter(seq_size, core_size), []
    while (w := it.next()) is not None:
        out.append(w[1:])
    return out


@pytest.fixture(scope="module")
def expected():
    """The nested loop of the reference, and what it says about the walk's harder cases."""
    E = collections.namedtuple("E", "hits windows speculated kept rescored triples pass_no_hit")
    hits, windows, speculated, kept, rescored, triples, pass_no_hit = [], 0, 0, 0, 0, 0, 0
    for p, K in enumerate(CORE_SIZES):
        for s, n in enumerate(READ_LENGTHS):
            spec = chain(n, K)
            speculated += len(spec)
            it, hit_idx = host.WindowIter(n, K), []
            while (w := it.next()) is not None:
                idx, start, stop = w
                windows += 1
                if hit_idx:  # after the pair's first hit: still the speculated window of this index, or a new one?
                    if idx < len(spec) and spec[idx] == (start, stop):
                        kept += 1
                    else:
                        rescored += 1
                outcome, lrt, pos = score(p, s, start, stop)
                pass_no_hit += outcome == PASS
                if outcome == HIT:
                    hits.append((p, s, idx, start, stop, float(lrt)))
                    hit_idx.append(idx)
                    it.set_last_hit_position(pos)
            triples += any(a + 1 == b and b + 1 == c for a, b, c in zip(hit_idx, hit_idx[1:], hit_idx[2:]))
    return E(hits, windows, speculated, kept, rescored, triples, pass_no_hit)


def test_cases_are_the_hard_ones(expected):
    assert expected.kept >= 100 and expected.rescored >= 100, (expected.kept, expected.rescored)
    assert expected.triples >= 3 and expected.pass_no_hit >= 1
    assert 0 in READ_LENGTHS and min(n for n in READ_LENGTHS if n) < 50 * min(CORE_SIZES)
    assert any(a == b for a, b in zip(READ_LENGTHS, READ_LENGTHS[1:]))
    assert any(n in READ_LENGTHS[:i - 1] and READ_LENGTHS[i - 1] != n for i, n in enumerate(READ_LENGTHS) if i > 1)
    assert len(expected.hits) > 100 and expected.windows != expected.speculated


def drive(plan, path_between=False):
    """Drives a walk as dcp_scan_run does: two chunks outstanding (the windows of chunk i + 1 are asked for before
    the results of chunk i are delivered), path batches once nothing is outstanding -- or, path_between, after every
    chunk -- and the rounds of what is left.  plan = None: nothing speculated.
    Returns (hits, windows walked, windows queued for scoring)."""
    walk = host.ScanWalk(CORE_SIZES, READ_LENGTHS)
    hits, queued = [], 0

    def path_batch():
        nonlocal queued
        wins = walk.take(walk.PATH)
        played = [score(*w) for w in wins.tolist()]
        assert all(o != BELOW for o, _, _ in played)
        found = walk.path_walked([o == HIT for o, _, _ in played], [pos for _, _, pos in played])
        for h in found:
            assert wins[h["batch_index"]].tolist() == [h["profile"], h["seq"], h["start"], h["stop"]]
            assert np.float32(h["lrt"]) == played[h["batch_index"]][1]
            hits.append((int(h["profile"]), int(h["seq"]), int(h["window"]), int(h["start"]), int(h["stop"]), float(h["lrt"])))
        queued += walk.take_queued()

    def passing(wins):
        played = [score(*w) for w in wins.tolist()]
        index = [k for k, (o, _, _) in enumerate(played) if o != BELOW]
        return index, [played[k][1] for k in index]

    if plan is None:
        walk.all_pairs()
        queued += walk.take_queued()
    else:
        chunks, windows = plan
        flight = collections.deque()

        def begin():
            nonlocal queued
            i = len(begun)
            begun.append(i)
            flight.append((chunks[i],) + walk.chunk_windows(chunks[i], windows[i]))
            queued += int(windows[i])

        begun = []
        while len(begun) < len(chunks) and len(flight) < 2:
            begin()
        while flight:
            chunk, wins, base = flight.popleft()
            if len(begun) < len(chunks):
                begin()
            walk.chunk_scored(chunk, base, *passing(wins))
            queued += walk.take_queued()
            while (path_between or not flight) and walk.waiting(walk.PATH):
                path_batch()
    while walk.waiting(walk.COST) or walk.waiting(walk.PATH):
        if walk.waiting(walk.PATH):
            path_batch()
        if walk.waiting(walk.COST):
            wins = walk.take(walk.COST)
            walk.cost_scored(*passing(wins))
            queued += walk.take_queued()
    return sorted(hits), walk.windows(), queued


def small_plan():
    """Many small chunks: a profile per chunk at the most, split by reads, and single pairs above the window cap."""
    cap = 64
    chunks, windows = host.plan_chunks(CORE_SIZES, READ_LENGTHS, 1.0e5, 1.0e5, 4, cap)
    assert len(chunks) > 3 * len(CORE_SIZES)
    over = windows > cap
    assert over.any() and ((chunks[over, 1] - chunks[over, 0]) * (chunks[over, 3] - chunks[over, 2]) == 1).all()
    return chunks, windows


@pytest.mark.parametrize("mode", ["one_chunk", "small_chunks", "small_chunks_path_between", "nothing_speculated"])
def test_walk_finds_the_reference_hits(expected, mode):
    if mode == "one_chunk":
        plan = host.plan_chunks(CORE_SIZES, READ_LENGTHS, FIRST_CELLS, float("inf"), PAIRS, CAP)
        assert len(plan[0]) == 1
    else:
        plan = None if mode == "nothing_speculated" else small_plan()
    hits, windows, queued = drive(plan, path_between=mode.endswith("path_between"))
    assert hits == expected.hits  # (profile, read, window, start, stop, lrt), in the reference's order
    assert windows == expected.windows
    # one progress callback per window scored: every speculated window and those scored again -- or simply every
    # window of the real chains when nothing is speculated
    assert queued == (expected.windows if plan is None else expected.speculated + expected.rescored)


def test_plan_and_chains_must_agree():
    walk = host.ScanWalk(CORE_SIZES, READ_LENGTHS)
    chunks, windows = host.plan_chunks(CORE_SIZES, READ_LENGTHS, FIRST_CELLS, float("inf"), PAIRS, CAP)
    for wrong in (int(windows[0]) - 1, int(windows[0]) + 1):
        with pytest.raises(host.HipError):
            walk.chunk_windows(chunks[0], wrong)
