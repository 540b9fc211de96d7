"""Windows at the edges of the path pass's blocks, shared by tests/test_emul_block_edges.py and
tests/test_gpu_block_edges.py.

A window's DP table is held a block at a time (deciphon_amd/csrc/dcp_types.h, restated in tests/path_layout.py):
checkpoints every B rows, block j recomputed over rows j B + 1 .. min(L, (j + 1) B + 5), the traceback handed over to
block j - 1 at the first stage <= lo = j B + 5.  B is a multiple of 5 and the row loops run five rows per turn, so what
can go wrong lies in the lengths around B + 5 (one block) and B + 6 (two, the upper one of a single row), in L mod 5 of
the window's last block, and in where a path stands when it is handed over: in which state, how far below lo, after a
step of which size.  The table holds, per B, the lengths of block_lengths(B) for one profile at the ragged end of every
class the path pass instantiates, all four (multi_hits, hmmer3_compat) modes, and a few profiles whose paths cross
boundaries inside insert runs; coverage() says what a run of it must have contained.

Pure numpy and seeded.  The oracle (tests/dcp_testlib.oracle) comes in as an argument where special transitions are
needed; which candidates end in a tie of the traceback is the emulator's to say: tests/test_emul_block_edges.py holds
TIED to what it finds."""
from collections import Counter, namedtuple
from functools import lru_cache

import numpy as np

from dcp_testlib import random_seq, synth_profile
from delete_run_cases import LAYOUT, MULTI_WAVE, SINGLE_WAVE, STRIP_KS
from path_layout import MB, block, budget_mb, literal_bytes, num_blocks, table_bytes

SEED = 2201
BLOCKS = (5, 10, 20)  # DECIPHON_HIP_CKPT_ROWS of the cases
GROUPS = (1, 2, 3)    # blocks side by side
STRIP = "strip"       # the class of K > 4096
READ = 96             # nucleotides per read: window i of a profile starts at nucleotide i
LITERAL_MAX = 128     # the reads of the strip class are that much longer: the windows of its literal pass (literal_rows)

# (Q, W, strips, K) of the emulator's strip shapes (tests/test_emul_strip_blocks.py): the strip class on the CPU
EMUL_STRIPS = ((1, 1, 3, 129), (2, 2, 2, 512), (4, 2, 2, 700), (1, 4, 2, 300))

# Candidates (profile, B, L) whose traceback ends in DCP_TB_TIE on the emulator: left out of the table.  The draw of SEED
# has none; tests/test_emul_block_edges.py::test_every_window_in_blocks fails when this is not what the emulator finds.
TIED = frozenset()
MAX_TIED = 0.05       # of the candidates, the share the emulator suites allow (tests/test_emul_kernels.py)


def block_lengths(B):
    """every residue of L mod 5 in a window of several blocks, both flips of the block count (B + 5 | B + 6 and
    2 B + 5 | 2 B + 6), an upper block of one row, one to four blocks"""
    want = (1, 4, 5, 6, B + 4, B + 5, B + 6, B + 7, B + 9, B + 10, B + 11, 2 * B + 5, 2 * B + 6) + \
           tuple(range(3 * B + 6, 3 * B + 11))
    return tuple(sorted(set(want)))


def class_sizes():
    """-> [((Q, W) or STRIP, K)]: the smallest profile of every class of the path pass (the last lane that owns a
    position owns a part of its Q), K = 61 on its 128 columns among them, then the strip class at one position in the
    third strip and at three whole strips.  The narrow cost shapes run the layout of their class here (LAYOUT)."""
    low = {}
    for Q, K in SINGLE_WAVE:
        shape = LAYOUT.get(Q, (Q, 1))
        low[shape] = min(low.get(shape, K), K)
    for Q, W, K in MULTI_WAVE:
        low[(Q, W)] = min(low.get((Q, W), K), K)
    return sorted(low.items(), key=lambda kv: kv[1]) + [(STRIP, K) for K in STRIP_KS[:2]]


Prof = namedtuple("Prof", "cls K prof read kind emul")  # emul: (Q, W, strips) of an emulator-only strip profile, or None
Case = namedtuple("Case", "pi B L a mode")              # window [a, a + L) of profile pi's read


def insert_rich(rng, K):
    """a profile whose best paths sit in insert states for rows on end: II and MI nearly free, the background cheaper than
    the null model and than any match"""
    prof = synth_profile(rng, K)
    f32 = np.float32
    prof.bg[:] = (prof.bg * f32(0.125)).astype(np.float32)
    prof.null[:] = (prof.null + f32(4.0)).astype(np.float32)
    prof.trans[2, : K - 1] = (prof.trans[2, : K - 1] * f32(0.25)).astype(np.float32)  # MI
    prof.trans[5, : K - 1] = (prof.trans[5, : K - 1] * f32(0.03125)).astype(np.float32)  # II
    return prof


@lru_cache(maxsize=None)
def profiles():
    """-> [Prof]: every fourth profile has the cheap MD / DD of the block tests (delete runs cross the boundaries)"""
    out = []
    sizes = class_sizes()
    for i, (cls, K) in enumerate(sizes):
        rng = np.random.default_rng([SEED, i])
        prof = synth_profile(rng, K)
        kind = "plain"
        if i % 4 == 0:
            prof.trans[7, 1:] = np.float32(0.01)
            prof.trans[3, 1:] = np.float32(0.02)
            kind = "deletes"
        out.append(Prof(cls, K, prof, random_seq(rng, READ + (LITERAL_MAX if cls == STRIP else 0)), kind, None))
    for i, (cls, K) in enumerate((((1, 1), 40), ((3, 1), 150), ((6, 2), 600))):  # hand-overs inside insert runs
        rng = np.random.default_rng([SEED, 100 + i])
        out.append(Prof(cls, K, insert_rich(rng, K), random_seq(rng, READ), "inserts", None))
    for i, (Q, W, S, K) in enumerate(EMUL_STRIPS):
        rng = np.random.default_rng([SEED, 200 + i])
        prof = synth_profile(rng, K)
        if i % 2 == 0:
            prof.trans[7, 1:] = np.float32(0.01)
            prof.trans[3, 1:] = np.float32(0.02)
        out.append(Prof(STRIP, K, prof, random_seq(rng, READ), "deletes" if i % 2 == 0 else "plain", (Q, W, S)))
    return out


def mode_of(L):
    """the (multi_hits, hmmer3_compat) mode of a window of L rows: bit 0 multi_hits, bit 1 hmmer3_compat.  By the
    amino length that selects the window's row of special transitions, so that one request holds all four (xt_table)"""
    return max(L // 3, 1) % 4


def xt_of(orc, L):
    m = mode_of(L)
    return orc.xtrans(max(L // 3, 1), m & 1, m >> 1)


def xt_table(orc, rows=128):
    """Engine.set_xtrans_table: row s in the mode of the windows of s amino acids"""
    table = np.zeros((rows, 13), np.float32)
    for s in range(1, rows):
        table[s] = orc.xtrans(s, (s % 4) & 1, (s % 4) >> 1)
    return table


def candidates(B):
    return [Case(pi, B, L, i, mode_of(L)) for pi in range(len(profiles())) for i, L in enumerate(block_lengths(B))]


def cases(B, gpu=False):
    """the table for blocks of B rows; gpu: without the emulator's own strip shapes"""
    return [c for c in candidates(B) if (c.pi, c.B, c.L) not in TIED and not (gpu and profiles()[c.pi].emul)]


def window(c):
    p = profiles()[c.pi]
    return p, np.ascontiguousarray(p.read[c.a : c.a + c.L])


def literal_rows(B):
    """-> (rows, budget in MB): the fewest rows, a multiple of 5, from which on a window of the strip class has two blocks
    or more and a whole table beyond a budget (whole MB, as DECIPHON_HIP_PATH_BUDGET_MB takes it) that holds a block's
    table, the checkpoints and the replay scratch of the windows up to five rows longer (tests/path_layout.py)"""
    rows = 5
    while True:
        rows += 5
        budget = max(budget_mb(literal_bytes(rows + 5, K, B, 1)) for K in STRIP_KS[:2])
        if num_blocks(rows + 1, B) >= 2 and all(budget * MB < table_bytes(rows + 1, K) for K in STRIP_KS[:2]):
            assert rows + 5 <= LITERAL_MAX
            return rows, budget


def literal_subset(B):
    """The cases of the literal pass on the GPU: one window per class and residue of L mod 5, of two blocks or more.  The
    strip class replays its trellis in blocks only under a budget below the whole table, so its windows here have
    literal_rows(B) + 1 .. + 5 rows, from the start of the profile's (longer) read.  A round of the replay is a thread's
    walk over K positions five times, and B = 5 has fourteen rounds: there K = 4097 alone (2.2 s for the test on an
    MI355X; 5.2 s with K = 6144 beside it, profiles/r22_block_edges.txt)."""
    seen, out = set(), []
    for c in cases(B, gpu=True):
        p = profiles()[c.pi]
        key = (c.pi, c.L % 5)
        if p.cls != STRIP and p.kind != "inserts" and num_blocks(c.L, B) >= 2 and key not in seen:
            seen.add(key)
            out.append(c)
    for pi, p in enumerate(profiles()):
        if p.cls == STRIP and not p.emul and (B > 5 or p.K == STRIP_KS[0]):
            rows = literal_rows(B)[0]
            out += [Case(pi, B, L, 0, mode_of(L)) for L in range(rows + 1, rows + 6)]
    return out


# ---- what a path does at the block boundaries ----
KINDS = ("M", "I", "D", "special")  # state id >> 14 (deciphon_amd/csrc/dcp_states.h)


def handovers(ids, sizes, L, B):
    """-> [(kind, lo - stage, size)] for the blocks above block 0, the highest first: the state with which the traceback
    of the path (steps in path order, S first) arrives at the first stage <= lo of the block, how far below lo that
    stage lies, and the emission length of the step that took it there"""
    ids, sizes = np.asarray(ids), np.asarray(sizes)
    stages = np.cumsum(sizes)  # the row a step's state is visited at
    assert stages[0] == 0 and stages[-1] == L
    out = []
    for j in range(num_blocks(L, B) - 1, 0, -1):
        lo = block(L, B, j).lo
        i = int(np.searchsorted(stages, lo, side="right")) - 1  # the last step at or below lo
        out.append((KINDS[int(ids[i]) >> 14], int(lo - stages[i]), int(sizes[i + 1])))
    return out


def coverage(items):
    """items: (class, K, B, L, ids, sizes) of every window of a run.  -> (counts, missing): what the windows contained,
    and the items of the list below that they did not --
      every size 1 .. 5 of the step that crosses a boundary;
      a hand-over 0 .. 4 rows below lo in a special state, in M and in D;
      one in I at lo and one below it;
      per class and B: every residue of L mod 5 among the windows of two or more blocks, and L = B + 5 and B + 6."""
    sizes_seen, landings, per = Counter(), Counter(), {}
    for cls, K, B, L, ids, sizes in items:
        got = per.setdefault(((cls, K), B), dict(residues=set(), lengths=set()))
        got["lengths"].add(L)
        if num_blocks(L, B) >= 2:
            got["residues"].add(L % 5)
        for kind, off, size in handovers(ids, sizes, L, B):
            assert 0 <= off <= 4 and 1 <= size <= 5 and off < size, (cls, K, B, L, kind, off, size)
            sizes_seen[size] += 1
            landings[(kind, off)] += 1
    missing = [("crossing size", s) for s in range(1, 6) if not sizes_seen[s]]
    missing += [("landing", k, o) for k in ("special", "M", "D") for o in range(5) if not landings[(k, o)]]
    if not landings[("I", 0)]:
        missing.append(("landing", "I", 0))
    if not any(landings[("I", o)] for o in range(1, 5)):
        missing.append(("landing", "I", "below lo"))
    for (cls, B), got in sorted(per.items(), key=str):
        missing += [("residue", cls, B, r) for r in range(5) if r not in got["residues"]]
        missing += [("length", cls, B, L) for L in (B + 5, B + 6) if L not in got["lengths"]]
    return dict(sizes=sizes_seen, landings=landings, per=per), missing
