"""CPU: the host half of scanning both strands -- the statement of a code row on either strand (dcp_code_rows_of,
include/deciphon_host.h: csrc/code_rows.h, what the kernels of csrc/code_rows.hip are built from and held to), the
scan's strand mode and its argument checks, which come before any device (dcp_scan_set_strands), the mapping of a row's hit back to the read as given (hit_on_read), and
the chunk planner and the window walk fed the doubled, interleaved read lengths a scan of both strands hands them."""
import numpy as np
import pytest

from deciphon_amd import hit_on_read, host

DCP_EFUNCUSE = 8
DCP_ESEQABC = 57
CODE_OFF = (0, 4, 20, 84, 340)
LENGTHS = list(range(12)) + [255, 256, 257, 513]


def rows_numpy(y) -> np.ndarray:
    """Row r, word t - 1: off[t] + the base-4 value of y[r-t..r-1], leftmost digit first; 0 where r < t."""
    y = np.asarray(y, np.int64)
    n = len(y)
    rows = np.zeros((n + 1, 8), np.uint32)
    for t in range(1, 6):
        for r in range(t, n + 1):
            v = 0
            for i in range(r - t, r):
                v = v * 4 + int(y[i])
            rows[r, t - 1] = CODE_OFF[t - 1] + v
    return rows


def rc(x) -> np.ndarray:
    return (3 - np.asarray(x, np.uint8)[::-1]).astype(np.uint8)


def palindrome(n: int, rng) -> np.ndarray:
    """A read that is its own reverse complement (even length)."""
    half = rng.integers(0, 4, n // 2).astype(np.uint8)
    return np.concatenate([half, rc(half)])


@pytest.mark.parametrize("n", LENGTHS)
def test_code_rows_of_both_strands(n):
    rng = np.random.default_rng(1000 + n)
    reads = [rng.integers(0, 4, n).astype(np.uint8), np.zeros(n, np.uint8), np.full(n, 3, np.uint8)]
    for x in reads:
        plus, minus = host.code_rows_of(x), host.code_rows_of(x, minus=True)
        assert plus.shape == minus.shape == (n + 1, 8)
        assert np.array_equal(plus, rows_numpy(x))
        assert np.array_equal(minus, rows_numpy(rc(x)))
        assert np.array_equal(minus, host.code_rows_of(rc(x)))
        assert not plus[:, 5:].any() and not minus[:, 5:].any()
    # all-A and all-T are each other's reverse complement
    assert np.array_equal(host.code_rows_of(reads[1], minus=True), host.code_rows_of(reads[2]))


@pytest.mark.parametrize("n", [0, 2, 4, 10, 256, 512])
def test_code_rows_of_reverse_palindrome(n):
    x = palindrome(n, np.random.default_rng(7 + n))
    assert np.array_equal(rc(x), x)
    assert np.array_equal(host.code_rows_of(x, minus=True), host.code_rows_of(x))


def test_code_rows_of_refuses():
    import ctypes as C

    L = host._lib()
    out = np.zeros((4, 8), np.uint32)
    bad = np.array([0, 1, 4], np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    for minus in (0, 1):
        assert L.dcp_code_rows_of(p(bad), 3, minus, p(out)) == DCP_ESEQABC
        assert L.dcp_code_rows_of(None, 3, minus, p(out)) == DCP_EFUNCUSE
        assert L.dcp_code_rows_of(p(bad), -1, minus, p(out)) == DCP_EFUNCUSE
        assert L.dcp_code_rows_of(p(bad), 2, minus, None) == DCP_EFUNCUSE
        assert L.dcp_code_rows_of(None, 0, minus, p(out)) == 0  # an empty read has one row
        assert not out[0].any()


def test_scan_strands_mode_needs_no_device(capfd):
    from deciphon_amd import scan

    L = scan._lib()
    assert L.dcp_scan_set_strands(None, 0) == DCP_EFUNCUSE
    assert L.dcp_scan_strands(None) == DCP_EFUNCUSE
    s = L.dcp_scan_new()
    assert s
    try:
        assert L.dcp_scan_strands(s) == 0  # plus is the default
        assert L.dcp_scan_set_strands(s, 1) == 0
        assert L.dcp_scan_strands(s) == 1
        for bad in (2, -1, 255):
            assert L.dcp_scan_set_strands(s, bad) == DCP_EFUNCUSE
            assert L.dcp_scan_strands(s) == 1  # a refused value changes nothing
        assert L.dcp_scan_set_strands(s, 0) == 0
        assert L.dcp_scan_strands(s) == 0
    finally:
        L.dcp_scan_del(s)
    capfd.readouterr()
    with pytest.raises(ValueError):
        scan.strands_code("minus")
    assert scan.strands_code("plus") == 0 and scan.strands_code("both") == 1


def test_hit_on_read():
    f = ["7", "0", "100", "900", "0", "20", "320", "PF1", "dna", "1.0", "nan", "ACG,M1,ACG,T"]
    assert hit_on_read("\t".join(f), 1000) == (120, 420, "+")  # 12 columns: a scan of the plus strand
    assert hit_on_read("\t".join(f + ["+"]), 1000) == (120, 420, "+")
    assert hit_on_read(f + ["+"], 1000) == (120, 420, "+")
    # [120, 420) of the reverse complement of a read of 1000 is [580, 880) of the read
    assert hit_on_read("\t".join(f + ["-"]), 1000) == (580, 880, "-")
    # a hit over the whole reverse complement is the whole read
    g = ["1", "0", "0", "30", "0", "0", "30", "PF1", "dna", "1.0", "nan", "x", "-"]
    assert hit_on_read(g, 30) == (0, 30, "-")
    # one nucleotide at the 5' end of the reverse complement is the read's last
    g[6] = "1"
    assert hit_on_read(g, 30) == (29, 30, "-")
    with pytest.raises(ValueError):
        hit_on_read(f + ["?"], 1000)


def _doubled(lengths):
    return np.repeat(np.asarray(lengths, np.int32), 2)


@pytest.mark.parametrize("limits", [(1e10, float("inf"), 1 << 21, 4 << 20), (3e4, 3e4, 5, 7), (1.0, 1.0, 1, 1)])
def test_planner_and_walk_on_interleaved_doubled_lengths(limits):
    K = np.array([3, 12, 40, 140], np.int32)
    lengths = [0, 1, 30, 601, 2500, 2500, 7001, 0, 64]
    R = _doubled(lengths)
    chunks, windows = host.plan_chunks(K, R, *limits)
    walk = host.ScanWalk(K, R)
    seen = {}
    for c, n in zip(chunks, windows):
        wins, base = walk.chunk_windows(c, int(n))
        assert base[-1] == n == len(wins)
        pairs = [(p, s) for p in range(c[0], c[1]) for s in range(c[2], c[3])]
        assert len(base) == len(pairs) + 1
        for i, (p, s) in enumerate(pairs):
            assert (p, s) not in seen  # every (profile, internal read) pair once
            w = wins[base[i] : base[i + 1]]
            assert (w[:, 0] == p).all() and (w[:, 1] == s).all()
            assert len(w) == host.window_count(int(R[s]), int(K[p]))
            seen[(p, s)] = w[:, 2:].copy()
    assert sorted(seen) == [(p, s) for p in range(len(K)) for s in range(len(R))]
    assert sum(len(v) for v in seen.values()) == int(windows.sum())
    # the windows of the minus strand of a read are those of its plus strand
    for p in range(len(K)):
        for s in range(len(lengths)):
            assert np.array_equal(seen[(p, 2 * s)], seen[(p, 2 * s + 1)])
