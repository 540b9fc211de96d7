"""GPU: a window list that is NOT in ascending profile order through the cost pass.  A scan sends its windows ascending,
which stages by counting passes; any other list is ordered by a comparison sort (deciphon_amd/csrc/stage_plan.h) that no
scan ever takes -- here it runs end to end on the device: packs, a narrow and a wide profile of one class, single-wave
classes, against the ascending list bit for bit and against the oracle."""
import numpy as np
import pytest

from dcp_testlib import bits, random_seq, synth_profile

pytestmark = pytest.mark.gpu


def test_shuffled_windows_cost_what_ascending_ones_do(engine, orc):
    rng = np.random.default_rng(23)
    profs = [synth_profile(rng, K, None, [0.0, 0.05][i % 2]) for i, K in enumerate((3, 100, 125, 173, 300, 350))]
    engine.clear_profiles()
    for p in profs:
        engine.add_profile(p.K, p.trans, p.match, p.null, p.bg)
    engine.commit()
    reads = [random_seq(rng, n) for n in (30, 41, 57, 64, 75, 90, 101, 120)]
    engine.set_sequences(reads)
    engine.set_mode(True, False)
    wins = np.array([(p, s, 0, len(r)) for p in range(len(profs)) for s, r in enumerate(reads)], np.int32)
    order = np.random.default_rng(1).permutation(len(wins))
    assert (np.diff(wins[:, 0]) >= 0).all() and (np.diff(wins[order, 0]) < 0).any()
    nul, alt = engine.cost(wins)
    snul, salt = engine.cost(wins[order])
    back = np.argsort(order)  # window j of the shuffled list is window order[j] of the ascending one
    assert np.array_equal(snul[back].view(np.uint32), nul.view(np.uint32))
    assert np.array_equal(salt[back].view(np.uint32), alt.view(np.uint32))
    for i, (p, s, a, b) in enumerate(wins):
        xt = orc.xtrans(max((b - a) // 3, 1), True, False)
        assert bits(nul[i]) == bits(orc.null(profs[p], xt, reads[s])), (profs[p].K, s)
        assert bits(alt[i]) == bits(orc.cost(profs[p], xt, reads[s])), (profs[p].K, s)
