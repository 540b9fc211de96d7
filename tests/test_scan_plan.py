"""CPU: how dcp_scan_run cuts profiles x reads into cost batches (dcp_window_count and dcp_scan_plan_chunks,
include/deciphon_host.h; the rules at csrc/host_logic.h dcp_plan_chunks).  A chunk holds every window of its pairs'
no-hit chains, so the planner must count them right and keep each chunk at or below the window cap -- unless the
chunk is a single pair, whose chain is never split -- for long reads and small profiles as well, where the windows
of one profile against all reads can exceed the cap many times over."""
import os
import re
import time

import numpy as np

from dcp_testlib import ROOT
from deciphon_amd import host, synth

HEADER = os.path.join(ROOT, "include", "deciphon_host.h")
FIRST_CELLS, PAIRS, CAP = 1.0e10, 1 << 21, 4 << 20  # what dcp_scan_run plans with by default


def walk(seq_size, core_size):
    """The no-hit chain's length by dcp_window_setup / dcp_window_next (c-core/window.c), one window at a time."""
    it, n = host.WindowIter(seq_size, core_size), 0
    while it.next() is not None:
        n += 1
    return n


def window_table(core_sizes, read_lengths):
    """int64[profiles][reads]: dcp_window_count of every pair (one call per distinct (K, length))."""
    memo = {}
    W = np.zeros((len(core_sizes), len(read_lengths)), np.int64)
    for p, K in enumerate(core_sizes):
        for s, n in enumerate(read_lengths):
            key = (int(K), int(n))
            if key not in memo:
                memo[key] = host.window_count(n, K)
            W[p, s] = memo[key]
    return W


def assert_plan(chunks, windows, core_sizes, read_lengths, first_cells, later_cells, max_pairs, max_windows):
    """Every rule of the plan: tiling in (profile, read) order, window counts, both caps, and that each chunk ends
    only where the next profile (or read) would break a limit."""
    K = np.asarray(core_sizes, np.int64)
    R = np.asarray(read_lengths, np.int64)
    nprof, nreads = len(K), len(R)
    W = window_table(K, R)
    per_profile = W.sum(axis=1)
    read_nt = float(R.sum())
    by_pairs = max(1, max_pairs // nreads) if nreads else max(nprof, 1)
    split = (per_profile > max_windows) | (nreads > max_pairs)  # the profiles that are cut by reads
    assert len(chunks) == len(windows)
    p, s = 0, 0
    for i, ((p0, p1, s0, s1), w) in enumerate(zip(chunks.tolist(), windows.tolist())):
        assert (p0, s0) == (p, s), f"chunk {i} leaves a gap or overlaps"
        assert p1 > p0 and (s1 > s0 or nreads == 0), i
        assert w == int(W[p0:p1, s0:s1].sum()), f"chunk {i}: {w} windows planned"
        assert w <= max_windows or (p1 - p0 == 1 and s1 - s0 == 1), f"chunk {i} above the cap: {w}"
        assert (p1 - p0) * (s1 - s0) <= max_pairs, i
        if split[p0]:
            assert p1 == p0 + 1, f"chunk {i}: a split profile is alone in its chunks"
            assert s1 - s0 <= max_pairs, i
            if s1 < nreads:  # the next read would break a cap
                assert s1 - s0 == max_pairs or w + W[p0, s1] > max_windows, f"chunk {i} ends early"
        else:
            assert (s0, s1) == (0, nreads) and not split[p0 + 1 : p1].any(), i
            cells = read_nt * float(K[p0:p1 - 1].sum()) if p1 - p0 > 1 else 0.0
            limit = first_cells if i == 0 else later_cells
            assert p1 - p0 == 1 or cells < limit, f"chunk {i} goes on past its cell limit"
            if p1 < nprof:  # the next profile would break a limit
                cells += read_nt * float(K[p1 - 1])
                assert (p1 - p0 == by_pairs or cells >= limit or w + per_profile[p1] > max_windows), \
                    f"chunk {i} ends early"
        p, s = (p1, 0) if s1 == nreads else (p0, s1)
    assert (p, s) == (nprof, 0), "the chunks do not reach the last pair"
    assert int(np.sum(windows)) == int(W.sum())
    return W


def test_header_holds_the_planners_defaults():
    defs = dict(re.findall(r"^#define (DCP_SCAN_\w+) (.+)$", open(HEADER).read(), re.M))
    assert float(defs["DCP_SCAN_FIRST_CHUNK_CELLS"]) == FIRST_CELLS
    assert eval(defs["DCP_SCAN_CHUNK_PAIRS"]) == PAIRS
    assert eval(defs["DCP_SCAN_CHUNK_WINDOWS"]) == CAP


def test_window_count_equals_the_window_walk_at_every_boundary():
    """dcp_window_count against the walk: K = 1 ... 16383 (the 50 K = 100000 span cap at K = 2000, the widest
    profile of a pressed database), lengths up to 3e5 at every span / step / 4 K boundary, and lengths of about
    1e7 where the chain is still a few thousand windows long.  The walk's start + span is int arithmetic, like
    c-core/window.c: everything here stays far below 2^31."""
    rng = np.random.default_rng(11)
    Ks = (1, 2, 3, 4, 5, 7, 10, 16, 24, 25, 26, 30, 49, 50, 99, 100, 173, 500, 1000, 1999, 2000, 2001, 2500,
          4096, 8192, 16383)
    checked = 0
    for K in Ks:
        span = min(50 * K, 100000)
        step = max(1, span + 1 - 4 * K)
        lengths = {1, 2, 3, 4 * K - 1, 4 * K, 4 * K + 1, 99999, 100000, 100001, 300000}
        for base in (span, span + step, span + 2 * step, span + 7 * step):
            lengths |= {base - 1, base, base + 1}
        lengths |= set(int(v) for v in rng.integers(1, 300001, size=4))
        for n in sorted(v for v in lengths if 1 <= v <= 300000):
            assert host.window_count(n, K) == walk(n, K), (n, K)
            checked += 1
        assert host.window_count(0, K) == walk(0, K) == 0
    for K in (30, 31, 173, 2001, 16383):
        for n in (9_999_991, 10_000_000, 12_345_679):
            assert host.window_count(n, K) == walk(n, K), (n, K)
            checked += 1
    assert checked > 500
    assert host.window_count(1000, 0) == 0 and host.window_count(-5, 10) == 0


def test_pfam_sized_database_against_long_contigs():
    """2e4 Pfam-shaped profiles against ten 10 Mb contigs and three empty reads: 3e8 windows in all, which the rule of
    old put into two chunks.  The plan tiles every pair once, in order, with no chunk above 4 Mi windows, and takes
    seconds at most."""
    K = synth.pfam_like_lengths(20000, 41)
    R = [10_000_000] * 5 + [0, 0] + [10_000_000 - 7 * i for i in range(5)] + [0]
    t = time.perf_counter()
    chunks, windows = host.plan_chunks(K, R, FIRST_CELLS, float("inf"), PAIRS, CAP)
    dt = time.perf_counter() - t
    assert dt < 5.0, f"planning took {dt:.1f} s"
    W = assert_plan(chunks, windows, K, R, FIRST_CELLS, float("inf"), PAIRS, CAP)
    assert W.sum() > 2e8
    assert len(chunks) > W.sum() // CAP and windows.max() <= CAP
    unbounded, _ = host.plan_chunks(K, R, FIRST_CELLS, float("inf"), PAIRS, 1 << 62)
    assert len(unbounded) == 2  # without the window cap: the first chunk, and all the rest in one


def test_small_profiles_split_by_reads_and_a_pair_above_the_cap_stands_alone():
    """K = 1 ... 3 against reads of 2e8 nt: one pair of K = 1 is 4.26 M windows, above the 4 Mi cap on its own (a chain
    is never split: its speculated scores must all be at hand when the pair hits).  Each such profile is cut by reads;
    a pair above the cap is a chunk of its own, the others share chunks at or below the cap."""
    K = [3, 1, 2, 40, 1]
    R = [200_000_000, 10_000_000, 0, 200_000_000, 5, 150_000_000, 7]
    chunks, windows = host.plan_chunks(K, R, FIRST_CELLS, float("inf"), PAIRS, CAP)
    W = assert_plan(chunks, windows, K, R, FIRST_CELLS, float("inf"), PAIRS, CAP)
    assert W[1, 0] == host.window_count(200_000_000, 1) > CAP
    big = [(c.tolist(), int(w)) for c, w in zip(chunks, windows) if w > CAP]
    assert big and all(c[1] - c[0] == 1 and c[3] - c[2] == 1 and c[0] in (1, 4) for c, _ in big)
    assert sum(1 for c in chunks if c[0] == 1) >= 3  # profile 1 in several chunks of reads
    assert [c.tolist() for c in chunks if c[0] == 3] == [[3, 4, 0, len(R)]]  # K = 40: 2e5 windows, whole


def test_small_caps_and_pair_limits():
    """The same rules with caps small enough to bind everywhere (what DECIPHON_HIP_CHUNK_WINDOWS sets), with cell
    limits on every chunk (DECIPHON_HIP_CHUNK_CELLS), and with more reads than pairs per chunk."""
    rng = np.random.default_rng(3)
    K = rng.integers(1, 300, size=60)
    R = [int(v) for v in rng.integers(0, 300_000, size=23)] + [0, 1_500_000, 1_400_000]
    for first, later, pairs, cap in ((FIRST_CELLS, float("inf"), PAIRS, 2000), (1e8, 1e8, PAIRS, 50_000),
                                     (5e9, float("inf"), 8, 30_000), (FIRST_CELLS, float("inf"), 30, 1)):
        chunks, windows = host.plan_chunks(K, R, first, later, pairs, cap)
        assert_plan(chunks, windows, K, R, first, later, pairs, cap)


def test_degenerate_inputs_and_errors():
    import ctypes as C

    chunks, windows = host.plan_chunks([], [100, 200], FIRST_CELLS, float("inf"), PAIRS, CAP)
    assert len(chunks) == 0
    chunks, windows = host.plan_chunks([5, 9, 7], [], FIRST_CELLS, float("inf"), PAIRS, CAP)
    assert chunks.tolist() == [[0, 3, 0, 0]] and windows.tolist() == [0]
    chunks, windows = host.plan_chunks([5, 9, 7], [0, 0], FIRST_CELLS, float("inf"), PAIRS, 1)
    assert chunks.tolist() == [[0, 3, 0, 2]] and windows.tolist() == [0]
    L = host._lib()
    K = np.array([1, 1, 1], np.int32)
    R = np.array([10_000, 10_000], np.int32)
    out = np.zeros((1, 4), np.int32)
    w = np.zeros(1, np.int64)
    n = C.c_int(0)
    args = (3, K.ctypes.data_as(C.c_void_p), 2, R.ctypes.data_as(C.c_void_p), FIRST_CELLS, float("inf"))
    ptrs = (out.ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p), C.byref(n))
    assert L.dcp_scan_plan_chunks(*args, PAIRS, 100, 1, *ptrs) == 20  # DCP_ENOMEM: 6 chunks, room for one
    assert n.value == 6 and out.tolist() == [[0, 0, 0, 0]]
    assert L.dcp_scan_plan_chunks(*args, PAIRS, 0, 1, *ptrs) == 8  # DCP_EFUNCUSE: no window cap
    assert L.dcp_scan_plan_chunks(*args, 0, 100, 1, *ptrs) == 8  # DCP_EFUNCUSE: no pair cap


def test_bench_headline_plan_is_the_rule_of_old():
    """bench.py's end-to-end scan (400 Pfam-shaped profiles x 500 reads of 10 kb) is planned exactly as before the
    window cap: a first chunk that stops once it holds 1e10 DP cells (the profile that crosses it included), then
    chunks of at most max(1, 2^21 / reads) profiles -- here one chunk of all the rest."""
    import bench

    K = synth.pfam_like_lengths(400, bench.SEED)
    nreads, read_len = 500, 10_000
    R = [read_len] * nreads
    # the rule dcp_scan_run applied before the planner
    read_nt = float(sum(R))
    by_pairs = max(1, PAIRS // nreads)
    old, p0 = [], 0
    while p0 < len(K):
        p1, cells = p0, 0.0
        limit = FIRST_CELLS if p0 == 0 else 1.0e300
        while p1 < len(K) and p1 - p0 < by_pairs and (p1 == p0 or cells < limit):
            cells += read_nt * float(K[p1])
            p1 += 1
        old.append([p0, p1, 0, nreads])
        p0 = p1
    chunks, windows = host.plan_chunks(K, R, FIRST_CELLS, float("inf"), PAIRS, CAP)
    assert chunks.tolist() == old
    assert len(old) == 2
    assert_plan(chunks, windows, K, R, FIRST_CELLS, float("inf"), PAIRS, CAP)
    assert int(windows.sum()) == len(bench.all_windows(K, nreads, read_len))
