"""GPU: the two lane vocabularies against each other, op by op.  deciphon_amd/csrc/lane_ops_gpu.h (DPP operands,
row_bcast steps in assembly with hand-counted wait states, ds_swizzle, readlane, structured buffer loads, LDS stashes
read in assembly, the Group<W> exchange through LDS records) and tests/emul/lane_ops_emul.h (the lock-step emulator
every test_emul_* suite stands on) run the same cases (tests/lanes/lane_cases.h) on the same seeded inputs
(tests/lane_conf_cases.py), and every output word -- per-lane results, uniform results in every lane, output memory --
must be the same bits; a NaN matches any NaN.  tests/test_lane_ops_emul.py holds the emulator's side against numpy, so
a difference here says which op of which side to read.  No case is exempt: the table is the library's own, and the
completeness guard of the CPU file ties it to what lane_ops_gpu.h declares."""
import numpy as np
import pytest

import lane_conf_cases as lc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def libs():
    return lc.gpu_lib(), lc.emul_lib()


def names():
    return sorted(lc.emul_lib().table())


def test_both_libraries_hold_the_same_table(libs):
    gpu, em = libs
    assert gpu.table() == em.table() and len(gpu.table()) >= 100


@pytest.mark.parametrize("name", names())
def test_gpu_against_emulator(libs, name):
    gpu, em = libs
    W, nin, nout, _ = em.table()[name]
    inp = lc.case_inputs(name, W, nin, nout)
    want, want_mem = em.run(name, inp)
    got, got_mem = gpu.run(name, inp)
    ok = lc.same_words(got, want)
    where = np.argwhere(~ok)  # (vector, output, lane)
    per_output = {int(j): int(n) for j, n in zip(*np.unique(where[:, 1], return_counts=True))}
    assert ok.all(), (name, per_output, where[:8].tolist(), [hex(x) for x in got[~ok][:8]], [hex(x) for x in want[~ok][:8]])
    ok = lc.same_words(got_mem, want_mem)
    where = np.argwhere(~ok)  # (vector, word)
    assert ok.all(), (name, "memory", len(where), where[:8].tolist(), [hex(x) for x in got_mem[~ok][:8]],
                      [hex(x) for x in want_mem[~ok][:8]])
