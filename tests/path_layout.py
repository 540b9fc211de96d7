"""What the path pass places in device memory, restated from the layout of deciphon_amd/csrc/dcp_types.h and the
rules of csrc/path_plan.h in plain arithmetic -- the check of the planner (test_path_plan.py) and the source of the
budgets of the GPU tests (test_gpu_strip_blocks.py), so nothing here calls the library.  K alone describes a profile of
the strip class (K > 4096: padded to strips of 2048 positions, eight wavefronts); the *_of functions take the padded
size Kp and the wavefronts W of any class."""
from collections import namedtuple

MB = 1 << 20
STRIP, WAVES = 2048, 8  # DCP_STRIP_POSITIONS; wavefronts of the strip kernels


def padded(K):
    return STRIP * ((K + STRIP - 1) // STRIP)


def num_blocks(L, B):
    return 1 if B <= 0 or L <= B + 5 else (L - 5 + B - 1) // B


def block_slots(L, B):
    return (L if B <= 0 or L <= B + 5 else B + 5) + 1


Block = namedtuple("Block", "row_base last lo first ckpt slots")


def block(L, B, j):
    """dcp_block: block j of a window of L rows -- the row it starts from, the last row it computes, the stage at or
    below which the traceback hands over to block j - 1 (-1: block 0), the first row the replay serves, the slot of its
    checkpoint (-1: from row 0), the rows of its table"""
    slots = block_slots(L, B)
    row_base = j * B
    last = L if L - row_base < slots else row_base + slots - 1
    lo = row_base + 5 if j > 0 else -1
    return Block(row_base, last, lo, lo + 1, j - 1, slots)


def aligned(nbytes, to=256):
    return (nbytes + to - 1) // to * to


def table_bytes_of(L, Kp):
    return (L + 1) * (8 + 3 * Kp) * 4


def block_table_bytes_of(L, Kp, B):
    return block_slots(L, B) * (8 + 3 * Kp) * 4


def ckpt_bytes_of(L, Kp, W, B, strip):
    """dcp_ckpt_floats: ring[10][Kp] and six lane rows per wavefront; dcp_strip_ckpt_floats: and B of five rows, padded to
    8 floats"""
    return (num_blocks(L, B) - 1) * (10 * Kp + 6 * 64 * W + (8 if strip else 0)) * 4


def group_tables_bytes_of(L, Kp, B, G):
    return aligned(min(G, num_blocks(L, B)) * block_table_bytes_of(L, Kp, B), 16)


def fast_bytes_of(L, Kp, W, B, G, strip):
    """G block tables and the checkpoints of one window, as the engine places them (a multiple of 256 bytes)"""
    return aligned(group_tables_bytes_of(L, Kp, B, G) + ckpt_bytes_of(L, Kp, W, B, strip))


def scratch_bytes(rows, K):
    """the replay scratch of the literal pass: 3 K floats per row of the trellis served"""
    return rows * 3 * K * 4


# ---- the strip class, by K ----
def table_bytes(L, K):
    return table_bytes_of(L, padded(K))


def block_table_bytes(L, K, B):
    return block_table_bytes_of(L, padded(K), B)


def ckpt_bytes(L, K, B):
    return ckpt_bytes_of(L, padded(K), WAVES, B, True)


def fast_bytes(L, K, B, G):
    return fast_bytes_of(L, padded(K), WAVES, B, G, True)


def literal_bytes(L, K, B, G):
    """the same with the replay scratch of G blocks: 3 K floats for each of the B + 6 rows a block can serve"""
    return fast_bytes(L, K, B, G) + aligned(scratch_bytes(min(G, num_blocks(L, B)) * (B + 6), K))


def budget_mb(nbytes):
    return nbytes // MB + 1
