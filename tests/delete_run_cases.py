"""Profiles with planted deletions, shared by tests/test_emul_delete_runs.py and tests/test_gpu_delete_runs.py.

A case is a profile of K positions and a read that matches positions 1..a and a+r+1..K codon by codon: the best
alignment deletes the r positions between them, so the D chain of every row behind position a carries one value
through the whole run -- across r / Q lane boundaries of a kernel that keeps Q positions per lane
(deciphon_amd/csrc/viterbi_body.h, dcp_lazy_turns_carry).  DD over the run is 0.0, tiny or whatever the random
profile holds ("ordinary": the carry dies after a few positions); `quant` rounds every other cost to a multiple of
it, which makes exact fp32 ties between the carried value and a lane's own chain common."""
import numpy as np

from dcp_testlib import CODE_OFF, synth_profile

LAZY_POSITIONS = 6  # DCP_LAZY_POSITIONS (viterbi_body.h): positions covered by the turns taken without a vote
LONG_RUN = 4 * LAZY_POSITIONS  # a run this long crosses four or more lane boundaries whatever the shape
TINY = np.float32(2.0 ** -20)
DD_KINDS = ("zero", "tiny", "ordinary")

# (Q, W of the kernel, K): every single-wave shape at the lower and the upper end of the profiles it serves
# (viterbi_kernels.hip, dcp_class_of and dcp_launch_cost_narrow: (5,1), (7,1), (10,1) run on the layouts of
# (6,1), (8,1), (6,2))
SINGLE_WAVE = ((1, 5), (1, 60), (2, 61), (2, 128), (3, 129), (3, 192), (4, 193), (4, 256), (5, 257), (5, 320),
               (6, 321), (6, 384), (7, 385), (7, 448), (8, 449), (8, 512), (10, 513), (10, 640))
LAYOUT = {5: (6, 1), 7: (8, 1), 10: (6, 2)}  # Q of the narrow kernels -> (Q, W) of the layout they read

# every shape of PackWave (S lanes per group, Q positions per lane), viterbi_kernels.hip
PACK_SHAPES = ((4, 1), (4, 2), (4, 4), (8, 2), (8, 4), (16, 2), (16, 3), (16, 4), (32, 2), (32, 3), (32, 4))


def run_lengths(K):
    """delete runs from 1 up to K - 2 positions, half of them LONG_RUN or longer where K allows"""
    want = (1, 3, LONG_RUN, LONG_RUN + 13, max(K // 2, LONG_RUN), K - 2)
    return sorted({r for r in want if 1 <= r <= K - 2})


def planted(rng, K, r, dd, quant=None, a=None):
    """-> (profile, read, a): the read matches positions 1..a and a+r+1..K (1-based), DD over the run is `dd`"""
    assert 1 <= r <= K - 2 and dd in DD_KINDS
    prof = synth_profile(rng, K, quant)
    if a is None:
        a = int(rng.integers(1, K - r))  # 1 <= a, a + r + 1 <= K
    codons = rng.integers(0, 64, size=K)
    low = np.float32(quant if quant else 0.25)
    for k in range(K):
        prof.match[CODE_OFF[2] + int(codons[k]), k] = low
    prof.trans[0, 1:] += np.float32(16.0)  # BM: entering behind the run costs more than deleting it
    prof.trans[1, 1:] = low                # MM
    prof.trans[3, a] = low                 # MD into the first deleted position (0-based a)
    prof.trans[6, a + r] = low             # DM out of the last one
    if dd != "ordinary":
        prof.trans[7, a + 1 : a + r + 1] = np.float32(0.0) if dd == "zero" else TINY
    kept = np.concatenate([codons[:a], codons[a + r :]])
    read = np.stack([kept // 16, (kept // 4) % 4, kept % 4], axis=1).reshape(-1).astype(np.uint8)
    return prof, read, a


def single_wave_cases():
    """-> [(Q, K, r, dd, quant)]"""
    return [(Q, K, r, dd, quant) for Q, K in SINGLE_WAVE for r in run_lengths(K) for dd in DD_KINDS
            for quant in (None, (1.0, 4.0)[r % 2])]
