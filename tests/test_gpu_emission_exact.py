"""GPU: every word the emission kernels write (emission_kernel, press_kernel.hip; reemit_kernel, press_reemit.hip;
one arithmetic, press_emission.h) against the exact model (tests/exact_emission.py), fp32 word by word.

press_emission.h promises "computed in double and rounded to fp32 once".  Held here: a word is -inf exactly where the
model's P is 0, never NaN or +inf, and otherwise the fp32 nearest the exact ln P.  The other fp32 neighbour passes only
where ln P lies within 2^-40 max(|ln P|, largest |ln term|) of the midpoint of the two -- a handful of double
operations err by about 2^-50 of the largest intermediate, which leaves 2^10 for the device's exp and log -- and for at
most one word in 10^5 of a case; a word two or more ulps off fails outright.  (tests/test_exact_emission.py shows on
the CPU that the formula in float64 needs the allowance for none of 88 660 words.)  Measured on an MI355X
(profiles/r18_emission_ulps.txt): every finite word of every case is the nearest, none takes the allowance; before
press_emission.h kept the exact parts of a 3-mer apart, 22 words did, at e = 1, 2^-24, 2^-25 and 1 - 2^-24, where a
3-mer's ln P lies beside fp32 midpoints by structure.

The entries are few, so the model stays cheap, and of every kind (hmm_testlib.edge_profile): the null and background
models, nodes as a real profile has them, a node with whole amino acids at probability 0, almost one-hot nodes at 60
and 200 nats for an amino acid of one codon and of six, a uniform node, and nodes 0, 63, 64, 65 and K - 1 of a K = 300
profile, which has a cost-order copy.  The grid is test_gpu_epsilon.py's and the three error rates where 1 - e taken
in fp32, or log(1 - e) for log1p(-e), shows: 2^-24, 2^-25 and the fp32 below 1.  Press is checked on the whole grid;
dcp_hip_load_hmm and dcp_hip_set_epsilon, which test_gpu_load_hmm.py and test_gpu_set_epsilon.py tie to press word
for word, at 0.1 and 1e-30, in the pool: sign flipped, headers, canonical rows and the cost-order copy."""
import numpy as np
import pytest

from dcp_testlib import TABLE_SIZE, choose_qw
from exact_emission import Entry
from hmm_testlib import EDGE_NODES, HMM, edge_profile, press
from test_gpu_epsilon import EPSILONS

pytestmark = pytest.mark.gpu

GRID = EPSILONS + (2.0 ** -24, 2.0 ** -25, 1.0 - 2.0 ** -24)
K_COPY = 300
COPY_NODES = (0, 63, 64, 65, K_COPY - 1)
ROW_HDR, COST_ORDER_HDR = 4, 32  # DCP_ROW_HDR, DCP_COST_ORDER_HDR (csrc/dcp_types.h)


class Case:
    """The .hmm, and per checked entry its exact model: (profile, entry of the profile, Entry); entry 0 = null
    model, 1 = background, 2 + k = the node of position k."""

    def __init__(self, d):
        from deciphon_amd import synth
        from deciphon_amd.host import HmmFile

        seeds = synth.load_hmm_seeds(HMM)
        (copied,) = synth.pfam_like_hmms(seeds, 1, 18, lengths=[K_COPY])
        self.hmm = str(d / "exact.hmm")
        synth.write_hmm(self.hmm, [edge_profile(seeds, np.random.default_rng(18)), copied])
        with HmmFile(self.hmm) as h:
            self.dist = [(p["nucltp"], p["codonm"]) for p in h]
        assert [len(n) - 3 for n, _ in self.dist] == [len(EDGE_NODES), K_COPY]
        for a, b in zip(self.dist[0], self.dist[1]):  # one null model and one background for the file
            assert np.array_equal(a[:2].view(np.uint32), b[:2].view(np.uint32))
        self.checked = [(0, i) for i in range(2 + len(EDGE_NODES))] + [(1, 2 + k) for k in COPY_NODES]
        assert len(self.checked) == 16
        self.entries = {pe: Entry(self.dist[pe[0]][0][pe[1]], self.dist[pe[0]][1][pe[1]]) for pe in self.checked}
        self.entries[1, 0], self.entries[1, 1] = self.entries[0, 0], self.entries[0, 1]
        self._rounded = {}
        # the kinds are there: a one-hot ATG, amino acids at probability 0 beyond the stops
        atg = 0 * 25 + 3 * 5 + 2
        for nats in (60, 200):  # ln P(ATG) = -19 e^-60, about: 0 in the host's fp32
            assert self.dist[0][1][2 + EDGE_NODES.index(("M", nats)), atg] == 0.0
        assert np.isneginf(self.dist[0][1][2 + EDGE_NODES.index("star")]).sum() > 3 * 8

    def rounded(self, profile, entry, e32):
        model = self.entries[profile, entry]
        key = (id(model), float(e32))
        if key not in self._rounded:
            self._rounded[key] = model.rounded(e32)
        return self._rounded[key]


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    return Case(tmp_path_factory.mktemp("emission_exact"))


class Tally:
    def __init__(self):
        self.words = self.finite = self.nearest = self.excused = 0

    def line(self, writer, e32):
        share = self.nearest / self.finite if self.finite else 1.0
        return (f"emission-exact writer={writer} epsilon={float(e32)!r} words={self.words} finite={self.finite} "
                f"nearest={self.nearest} share={share:.6f} excused={self.excused}")

    def finish(self, writer, e32):
        print(self.line(writer, e32))
        assert self.excused * 100000 <= self.words, self.line(writer, e32)


def check_words(case, profile, entry, e32, got, where, tally):
    """got: float32[1364], log-probabilities as written for the entry"""
    want = case.rounded(profile, entry, e32)
    where = f"{where}, profile {profile} entry {entry} at epsilon {float(e32)!r}"
    assert got.dtype == np.float32 and got.shape == (TABLE_SIZE,)
    assert not np.isnan(got).any() and not np.isposinf(got).any(), where
    wrong_inf = np.isneginf(got) != want.zero
    assert not wrong_inf.any(), f"{where}: code {int(np.flatnonzero(wrong_inf)[0])} is -inf where P > 0, or the reverse"
    live = ~want.zero
    nearest = live & (got == want.nearest)
    other = live & ~nearest & (got == want.other)
    far = np.flatnonzero(live & ~nearest & ~other)
    assert len(far) == 0, (f"{where}: {len(far)} words two or more ulps off, first code {int(far[0])}: {got[far[0]]!r} "
                           f"for ln P = {want.lnp[far[0]]!r} between {want.below[far[0]]!r} and {want.above[far[0]]!r}")
    for code in np.flatnonzero(other):
        x = abs(want.lnp[code])
        scale = max(x, case.entries[profile, entry].largest_term(e32, int(code)))
        assert want.mid_rel[code] * x <= 2.0 ** -40 * scale, (
            f"{where}: code {int(code)} is {got[code]!r}, the nearest fp32 of ln P = {want.lnp[code]!r} is "
            f"{want.nearest[code]!r}; ln P is {want.mid_rel[code]:.3g} |ln P| from the midpoint, "
            f"{int(other.sum())} such words in this entry")
    tally.words += TABLE_SIZE
    tally.finite += int(live.sum())
    tally.nearest += int(nearest.sum())
    tally.excused += int(other.sum())


@pytest.mark.parametrize("epsilon", GRID)
def test_press_writes_the_nearest_fp32(case, tmp_path, epsilon):
    from deciphon_amd.host import Database

    e32 = np.float32(epsilon)
    db = Database(press(case.hmm, str(tmp_path / "exact.dcp"), 1, float(e32)))
    assert db.epsilon == e32 and len(db) == 2
    tally = Tally()
    for i in range(2):
        p = db.protein(i)
        # the inputs the kernel took, as stored: the distributions the model was made from
        assert np.array_equal(p["nucltp"].view(np.uint32), case.dist[i][0].view(np.uint32))
        assert np.array_equal(p["codonm"].view(np.uint32), case.dist[i][1].view(np.uint32))
        tables = np.concatenate([p["null_emission"][None], p["bg_emission"][None], p["emission"]])
        for profile, entry in case.checked:
            if profile == i:
                check_words(case, i, entry, e32, tables[entry], "press", tally)
    db.close()
    assert tally.words == 16 * TABLE_SIZE
    if epsilon in (0.0, 1.0):
        assert 0 < tally.finite <= 16 * 64  # whole codons alone, or the four-error term of a 3-mer alone
    else:
        assert tally.finite > 8 * TABLE_SIZE
    tally.finish("press", e32)


def canonical_floats(Kp):
    """rows[1364][DCP_ROW_HDR + Kp] and trans[8][Kp] of a profile in the pool, rounded up to 32 floats"""
    return (TABLE_SIZE * (ROW_HDR + Kp) + 8 * Kp + 31) & ~31


def check_pool(case, e32, writer, eng, tally):
    """Profiles 0 and 1 as they lie in the pool: costs, so the sign flipped back; the headers of every row, the
    checked nodes' columns of the canonical rows and, for the K = 300 profile, of the cost-order copy."""
    from deciphon_amd import host

    inf = np.float32(np.inf)
    assert [eng.core_size(i) for i in range(2)] == [len(EDGE_NODES), K_COPY]
    for i, K in enumerate((len(EDGE_NODES), K_COPY)):
        w = eng.profile_tables(i)
        Q, W = choose_qw(K)
        Kp = 64 * Q * W
        cols, stride = host.cost_order_map(5, 1) if i == 1 else (None, 0)  # K = 257..320: the copy of shape (5, 1)
        assert len(w) == canonical_floats(Kp) + TABLE_SIZE * stride, (K, len(w))
        views = [("canonical rows", w[: TABLE_SIZE * (ROW_HDR + Kp)].reshape(TABLE_SIZE, ROW_HDR + Kp), ROW_HDR,
                  np.arange(Kp))]
        if i == 1:
            assert stride == COST_ORDER_HDR + 64 * 5 and len(cols) == 64 * 5
            copy = w[canonical_floats(Kp):].reshape(TABLE_SIZE, stride)
            assert (copy[:, ROW_HDR:COST_ORDER_HDR] == inf).all()
            views.append(("cost-order copy", copy, COST_ORDER_HDR, cols))
        for name, rows, hdr, col in views:
            assert (rows[:, 2:ROW_HDR] == 0.0).all(), name
            check_words(case, i, 0, e32, -rows[:, 0], f"{writer}, null header of the {name}", tally)
            check_words(case, i, 1, e32, -rows[:, 1], f"{writer}, background header of the {name}", tally)
            for profile, entry in case.checked:
                if profile == i and entry >= 2:
                    k = entry - 2
                    check_words(case, i, entry, e32, -rows[:, hdr + col[k]], f"{writer}, position {k} of the {name}",
                                tally)
            pad = np.ones(rows.shape[1], bool)
            pad[:hdr] = False
            pad[hdr + np.asarray(col[:K])] = False
            assert (rows[:, pad] == inf).all(), name  # behind K: +inf


@pytest.mark.parametrize("writer", ["load_hmm", "set_epsilon"])
@pytest.mark.parametrize("epsilon", [0.1, 1e-30])
def test_the_pool_holds_the_nearest_fp32(case, monkeypatch, epsilon, writer):
    import deciphon_amd

    monkeypatch.delenv("DECIPHON_HIP_COST_ORDER", raising=False)
    e32 = np.float32(epsilon)
    tally = Tally()
    with deciphon_amd.Engine(0) as eng:
        if writer == "load_hmm":
            eng.load_hmm(case.hmm, 1, float(e32))
        else:
            eng.load_hmm(case.hmm, 1, 0.01)
            eng.set_epsilon(float(e32))
        assert eng.profile_epsilon(0) == e32 and eng.profile_epsilon(1) == e32
        check_pool(case, e32, writer, eng, tally)
    # null and background in each layout, the nine nodes, and the five nodes of the copied profile twice
    assert tally.words == (2 + 9 + 2 + 5 + 2 + 5) * TABLE_SIZE
    tally.finish(writer, e32)
