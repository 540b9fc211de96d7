"""CPU: the cost-order copy of the emission rows (dcp_cost_order_map, include/deciphon_host.h).  For every cost shape
the map is a bijection of the 64 Q W positions onto the columns [0, 64 Q W), the identity for Q <= 4, and every chunk
load of a wave -- chunk c = q / 4 of each of its 64 lanes, four floats or the narrower tail -- reads one contiguous
span of 64 x width floats, in lane order, aligned to 128 bytes."""
import numpy as np
import pytest

from deciphon_amd import host

# every (Q, W) a cost kernel runs, the narrow shapes included, and a few more
SHAPES = [(1, 1), (2, 1), (3, 1), (4, 1), (5, 1), (6, 1), (7, 1), (8, 1), (10, 1), (6, 2), (4, 4), (6, 4), (8, 4),
          (8, 8), (5, 2), (7, 3), (9, 1), (3, 2)]


@pytest.mark.parametrize("Q,W", SHAPES)
def test_map_is_a_bijection(Q, W):
    cols, stride = host.cost_order_map(Q, W)
    Kc = 64 * Q * W
    assert cols.shape == (Kc,)
    assert np.array_equal(np.sort(cols), np.arange(Kc))
    # the row: the { null, bg, 0, 0 } header padded to 128 bytes, then the columns; rows stay 128-byte aligned
    assert stride == 32 + Kc and stride % 32 == 0


@pytest.mark.parametrize("Q,W", [s for s in SHAPES if s[0] <= 4])
def test_identity_up_to_four_positions(Q, W):
    cols, _ = host.cost_order_map(Q, W)
    assert np.array_equal(cols, np.arange(64 * Q * W))


@pytest.mark.parametrize("Q,W", SHAPES)
def test_every_chunk_of_a_wave_is_one_span(Q, W):
    cols, _ = host.cost_order_map(Q, W)
    k = np.arange(64 * Q * W)
    g, q = k // Q, k % Q
    wave, lane = g // 64, g % 64
    spans = []
    for w in range(W):
        for c in range((Q + 3) // 4):
            wc = min(4, Q - 4 * c)
            # lane e's floats of chunk c, lane by lane: one run of consecutive columns
            sel = (wave == w) & (q // 4 == c)
            order = np.lexsort((q[sel], lane[sel]))
            got = cols[sel][order]
            assert len(got) == 64 * wc
            assert np.array_equal(got, got[0] + np.arange(64 * wc)), (w, c)
            # and it starts where a load of that width is aligned
            assert got[0] % 4 == 0 and (got[0] * 4) % 128 == 0
            spans.append((got[0], got[0] + 64 * wc))
    spans.sort()
    assert spans[0][0] == 0 and all(a[1] == b[0] for a, b in zip(spans, spans[1:]))


def test_refuses_shapes_beyond_a_workgroup():
    for Q, W in [(0, 1), (1, 0), (8, 16)]:
        with pytest.raises(ValueError):
            host.cost_order_map(Q, W)
