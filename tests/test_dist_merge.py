"""CPU: the merge rule of a scan whose reads are sharded (deciphon_amd.dist.merge_read_shards) on hand-made rows, and
the header scan_partitioned writes."""
import numpy as np
import pytest

from deciphon_amd import dist as ddist


def test_merge_read_shards():
    merge = ddist.merge_read_shards
    # three ranks; rank 1 found nothing; profile 1 only on rank 2; profile 5 only on rank 0
    rows = [["p0 r0 a", "p0 r0 b", "p2 r1", "p5 r0"], [], ["p0 r7", "p1 r8", "p2 r7", "p2 r9"]]
    prof = [np.array([0, 0, 2, 5], np.int32), np.zeros(0, np.int32), np.array([0, 1, 2, 2], np.int32)]
    assert merge(rows, prof) == ["p0 r0 a", "p0 r0 b", "p0 r7", "p1 r8", "p2 r1", "p2 r7", "p2 r9", "p5 r0"]
    assert merge([[], [], []], [[], [], []]) == []
    assert merge([], []) == []
    # equal profile indices stay in rank order, and within a rank in the rank's own order
    assert merge([["b", "a"], ["d", "c"]], [[3, 3], [3, 3]]) == ["b", "a", "d", "c"]
    assert merge([["x"]], [[0]]) == ["x"]
    with pytest.raises(ValueError):
        merge([["x"]], [[0, 1]])


def test_products_header_follows_the_strands():
    assert ddist.products_header("plus") == ddist.PRODUCTS_HEADER
    assert ddist.products_header("both") == ddist.PRODUCTS_HEADER + "\tstrand"
