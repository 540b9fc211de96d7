"""CPU: which columns of an emission row the lanes of a cost kernel read (dcp_row_lane_offsets,
include/deciphon_host.h; deciphon_amd/csrc/dcp_types.h dcp_row_read_offset) -- for every shape the engine launches and
every core size K the shape can be given.  A lane that owns a position below K reads where it always did (the lane
offset 16 + 4 Q e of the canonical rows, chunk c of it 16 bytes on; the contiguous spans of the cost-order copy; a
pack's column offset), a lane that owns none reads with the last lane that does, so nothing is read beyond that lane's
last byte, and a pack's separator lane reads the row's header."""
import numpy as np
import pytest

from deciphon_amd import host

ROW_HDR_BYTES = 16         # { null, bg, 0, 0 } in front of the canonical rows
COST_ORDER_HDR_BYTES = 128 # the header of a cost-order row, padded to a line

CANON_Q = (1, 2, 3, 4, 5, 6, 7, 8, 10)
ORDERED_Q = (5, 6, 7, 8, 10)
PACK_SHAPES = ((1, 4), (2, 4), (4, 4), (2, 8), (4, 8), (2, 16), (3, 16), (4, 16), (2, 32), (3, 32), (4, 32))


def widths(Q):
    return [min(4, Q - 4 * c) for c in range((Q + 3) // 4)]


def canon_offsets(Q):
    """row_lane_offset and, chunk by chunk, row_chunk_offsets on the canonical rows: uint32[64][chunks]"""
    e = np.arange(64, dtype=np.int64)[:, None]
    c = np.arange((Q + 3) // 4, dtype=np.int64)[None, :]
    return ROW_HDR_BYTES + 4 * Q * e + 16 * c


def ordered_offsets(Q):
    """row_chunk_offsets on the cost-order copy of one wavefront: uint32[64][chunks]"""
    e = np.arange(64, dtype=np.int64)[:, None]
    c = np.arange((Q + 3) // 4, dtype=np.int64)[None, :]
    return COST_ORDER_HDR_BYTES + 1024 * c + 4 * e * np.array(widths(Q), np.int64)[None, :]


def check_wave(layout, Q, today):
    w = np.array(widths(Q), np.int64)
    for K in range(1, 64 * Q + 1):
        real, off = host.row_lane_offsets(layout, Q, 0, K)
        off = off.astype(np.int64)
        assert real == min(64, -(-K // Q)), K
        assert off.shape == today.shape
        # lanes with a position below K: exactly today's offsets, the lane that straddles K included
        assert np.array_equal(off[:real], today[:real]), K
        # the others: with the last such lane, chunk by chunk -- so nothing beyond that lane's last byte
        assert np.array_equal(off[real:], np.broadcast_to(today[real - 1], off[real:].shape)), K
        assert ((off + 4 * w) <= (today[real - 1] + 4 * w)).all(), K
        assert (off + 4 * w).max() == (today[real - 1] + 4 * w).max(), K


@pytest.mark.parametrize("Q", CANON_Q)
def test_canonical_rows(Q):
    check_wave(host.ROW_CANON, Q, canon_offsets(Q))
    # one load of Q floats (Q <= 4, the table-writing kernels) starts where chunk 0 does
    assert np.array_equal(canon_offsets(Q)[:, 0], ROW_HDR_BYTES + 4 * Q * np.arange(64))


@pytest.mark.parametrize("Q", ORDERED_Q)
def test_cost_order_copy(Q):
    today = ordered_offsets(Q)
    # the copy's own map says the same: chunk c of lane e starts at the column of position e Q + 4 c
    cols, _ = host.cost_order_map(Q, 1)
    e = np.arange(64)[:, None]
    c = np.arange((Q + 3) // 4)[None, :]
    assert np.array_equal(today, COST_ORDER_HDR_BYTES + 4 * cols[e * Q + 4 * c].astype(np.int64))
    check_wave(host.ROW_COST_ORDER, Q, today)


@pytest.mark.parametrize("Q,S", PACK_SHAPES)
def test_packs(Q, S):
    e = np.arange(S, dtype=np.int64)
    today = ROW_HDR_BYTES + 4 * Q * (e - 1)  # the column offset of lane e >= 1: positions (e - 1) Q ..
    for K in range(1, (S - 1) * Q + 1):
        real, off = host.row_lane_offsets(host.ROW_PACK, Q, S, K)
        off = off.astype(np.int64)[:, 0]
        assert real == -(-K // Q) and 1 <= real <= S - 1, K
        assert off[0] == 0, K  # the separator: the row's header
        assert np.array_equal(off[1 : real + 1], today[1 : real + 1]), K
        assert (off[real + 1 :] == today[real]).all(), K  # with the group's last lane that owns a position
        assert (off[1:] + 4 * Q).max() == today[real] + 4 * Q, K


def test_refuses_what_no_kernel_has():
    for layout, Q, S, K in [(0, 0, 0, 1), (0, 3, 0, 0), (0, 3, 0, 193), (1, 17, 0, 5), (2, 3, 5, 4), (2, 3, 16, 46),
                            (3, 3, 0, 10)]:
        with pytest.raises(ValueError):
            host.row_lane_offsets(layout, Q, S, K)
