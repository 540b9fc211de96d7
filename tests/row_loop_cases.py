"""Cases shared by tests/test_emul_row_loop_ends.py and tests/test_gpu_row_loop_ends.py: the two ends of the cost
kernels' row loop (deciphon_amd/csrc/viterbi_body.h CostWave::run, viterbi_pack.h PackWave::run).

The loop runs five rows per iteration and one to four rows behind it, every row asks for the next row's emissions
and the codes of the row after that, the last row included (the code row is clamped to the window's last), and the
k-1 shifts put 0 -- not +inf -- into the first lane, where the kernel itself sets MM, MD, IM, DM and DD to +inf.
So what can go wrong shows in the first and last rows of a window, and at k = 0 of the transition tables."""
import numpy as np

# window lengths: every L up to two and a half iterations, then every residue of L mod 5 around three larger lengths
WINDOW_LENGTHS = tuple(range(1, 13)) + tuple(range(33, 38)) + tuple(range(58, 63)) + tuple(range(120, 125))

# k = 0 of MM, MD, IM, DM, DD (rows 1, 3, 4, 6, 7 of trans[8][K]): position 0 has no k-1 neighbour and the kernels
# never let these entries reach a score.  The engine refuses negative delete costs wherever they stand
# (dcp_hip_add_profile), so MD and DD take the non-negative junk only.
K0_ROWS = (1, 3, 4, 6, 7)
K0_JUNK = ((0.0, 0.0, 0.0, 0.0, 0.0), (-3.5, 0.0, -0.25, -17.0, 1.5), (1e-30, 2.0, -1e30, 7.0, 0.0),
           (-0.0, 1e30, 0.5, -1.0, 3.0e-3))


def with_k0(prof, junk):
    """a copy of `prof` with trans[K0_ROWS, 0] = junk (None: +inf, the form protein_setup_viterbi leaves)"""
    trans = np.array(prof.trans, np.float32, copy=True)
    trans[list(K0_ROWS), 0] = np.float32(np.inf) if junk is None else np.asarray(junk, np.float32)
    return type(prof)(prof.K, trans, prof.match, prof.null, prof.bg, prof.accession)
