"""CPU: the exact emission model (tests/exact_emission.py) and what "computed in double and rounded to fp32 once"
(csrc/press_emission.h) means, before a GPU is involved.

The exact model is the model: it equals dcp_testlib.emission_probs (oracle/pydecode.py: emission_prob over tables) to
1e-12 in probability.  It is not log(emission_probs): on an almost one-hot entry the float64 probability form, f = 1 -
e and f**4 M, lands hundreds of fp32 ulps from ln P once e is small, so no test of the kernels' words may compare
against it.  A float64 restatement of the kernels' own formula -- log-space terms, log1p(-e), a max-shifted sum -- gives
the nearest fp32 of the exact ln P on every entry of a grid: that is the bound tests/test_gpu_emission_exact.py holds
the kernels to.  decimal and mpmath agree."""
import os

import numpy as np
import pytest

import exact_emission
from dcp_testlib import CODE_DIGITS, GOLDEN, TABLE_SIZE, emission_probs
from exact_emission import Entry
from hmm_testlib import EDGE_NODES, HMM, edge_profile

ANY = 4
ATG = 20 + 0 * 16 + 3 * 4 + 2  # A, C, G, T = 0, 1, 2, 3; 3-mers start at code 20
EPSILONS = (0.0, 1.4e-45, 1e-30, 1e-12, 1e-4, 0.01, 0.1, 0.5, 0.999, 1.0)
# where ln P of a 3-mer lies beside the midpoint of two fp32 values by structure: 4 ln(1 - e) = -2^-22 and -2^-23
TIE_PRONE = (2.0 ** -24, 2.0 ** -25, 1.0 - 2.0 ** -24)


def narrow_sum(base, small) -> np.ndarray:
    """dcp_emission::narrow_sum: the fp32 nearest base + small, by way of the double sum rounded to odd."""
    base, small = np.broadcast_arrays(np.asarray(base, np.float64), np.asarray(small, np.float64))
    total = base + small
    err = np.where(np.abs(base) >= np.abs(small), small - (total - base), base - (total - small))
    bits = total.view(np.int64).copy()
    move = np.isfinite(total) & (err != 0.0) & (bits & 1 == 0)
    bits[move] += np.where((err > 0.0) == (total > 0.0), 1, -1)[move]
    return bits.view(np.float64).astype(np.float32)


def kernel_formula(epsilon, nucltp, codonm) -> np.ndarray:
    """dcp_emission::emission_lprob (csrc/press_emission.h) for the 1364 codes of one entry, in float64 with numpy's
    exp, log and log1p, rounded to fp32 at the end: the same terms, sums in the same order, the same max-shifted
    log_sum, and for a 3-mer the same split into exact parts and narrow_sum.  -> float32[1364]"""
    lp = np.asarray(nucltp, np.float32).astype(np.float64).reshape(4)
    lm = np.asarray(codonm, np.float32).astype(np.float64).reshape(5, 5, 5)
    p, M = np.exp(lp), np.exp(lm)
    e = np.float64(np.float32(epsilon))
    log = np.log

    def del1(a, b):
        return M[ANY, a, b] + M[a, ANY, b] + M[a, b, ANY]

    def one(a):
        return M[a, ANY, ANY] + M[ANY, a, ANY] + M[ANY, ANY, a]

    def m3(r):
        return M[r[:, 0], r[:, 1], r[:, 2]]

    def log_sum(*terms):
        hi = np.maximum.reduce(terms)
        none = np.isneginf(hi)
        shift = np.where(none, 0.0, hi)
        total = np.exp(terms[0] - shift)
        for t in terms[1:]:
            total = total + np.exp(t - shift)
        return np.where(none, -np.inf, hi + log(total))

    out, out32 = np.empty(TABLE_SIZE), np.empty(TABLE_SIZE, np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        le, lf = log(e), np.log1p(-e)
        z = CODE_DIGITS[0]
        out[0:4] = log(1.0 / 3.0) + 2.0 * le + 2.0 * lf + log(one(z[:, 0]))
        z0, z1 = CODE_DIGITS[1].T
        out[4:20] = log_sum(log(2.0 / 3.0) + le + 3.0 * lf + log(del1(z0, z1)),
                            log(1.0 / 3.0) + 3.0 * le + lf + log(p[z0] * one(z1) + p[z1] * one(z0)))
        z0, z1, z2 = CODE_DIGITS[2].T
        # a 3-mer: each term as (what e gives) + (what the inputs give); the largest keeps its parts apart
        e_part = [4.0 * lf, log(4.0 / 9.0) + 2.0 * le + 2.0 * lf, 4.0 * le]
        i_part = [lm[z0, z1, z2], log(p[z0] * del1(z1, z2) + p[z1] * del1(z0, z2) + p[z2] * del1(z0, z1)),
                  lp[z0] + lp[z1] + lp[z2]]
        t = np.array([e_part[i] + i_part[i] for i in range(3)])
        hi = t.max(axis=0)
        none = np.isneginf(hi)
        top = np.where(t[0] == hi, 0, np.where(t[1] == hi, 1, 2))
        others = np.exp(t - np.where(none, 0.0, hi))
        others[top, np.arange(64)] = 0.0
        # (the kernel adds the two others in the order of their indices, as this sum over three with a zero does)
        small = np.choose(top, e_part) + np.log1p(others[0] + others[1] + others[2])
        out32[20:84] = np.where(none, np.float32(-np.inf), narrow_sum(np.choose(top, i_part), small))
        z = CODE_DIGITS[3]
        a = (p[z[:, 0]] * m3(z[:, [1, 2, 3]]) + p[z[:, 1]] * m3(z[:, [0, 2, 3]]) + p[z[:, 2]] * m3(z[:, [0, 1, 3]]) +
             p[z[:, 3]] * m3(z[:, [0, 1, 2]]))
        b = 0.0
        for i in range(4):
            for j in range(i + 1, 4):
                r = np.delete(z, (i, j), axis=1)
                b = b + p[z[:, i]] * p[z[:, j]] * del1(r[:, 0], r[:, 1])
        out[84:340] = log_sum(log(1.0 / 2.0) + le + 3.0 * lf + log(a), log(1.0 / 9.0) + 3.0 * le + lf + log(b))
        z = CODE_DIGITS[4]
        v = 0.0
        for i in range(5):
            for j in range(i + 1, 5):
                v = v + p[z[:, i]] * p[z[:, j]] * m3(np.delete(z, (i, j), axis=1))
        out[340:] = log(1.0 / 10.0) + 2.0 * le + 2.0 * lf + log(v)
    threes = out32[20:84].copy()
    out32[:] = out
    out32[20:84] = threes
    return out32


@pytest.fixture(scope="module")
def entries(tmp_path_factory):
    """{name: (nucltp[4], codonm[125], Entry)}: null, background and two nodes of minifam.dcp, and an almost one-hot
    node (M; every other amino acid at e^-60), as the host makes its distributions from a HMMER3 file."""
    from deciphon_amd import synth
    from deciphon_amd.host import Database, HmmFile

    db = Database(os.path.join(GOLDEN, "minifam.dcp"))
    p = db.protein(0)
    picked = {"null": (p["nucltp"][0], p["codonm"][0]), "background": (p["nucltp"][1], p["codonm"][1]),
              "node 1": (p["nucltp"][2 + 1], p["codonm"][2 + 1]), "node 40": (p["nucltp"][2 + 40], p["codonm"][2 + 40])}
    db.close()
    hmm = str(tmp_path_factory.mktemp("exact") / "edge.hmm")
    synth.write_hmm(hmm, [edge_profile(synth.load_hmm_seeds(HMM), np.random.default_rng(7))])
    with HmmFile(hmm) as h:
        (edge,) = list(h)
    k = EDGE_NODES.index(("M", 60))
    picked["one-hot"] = (edge["nucltp"][2 + k], edge["codonm"][2 + k])
    assert picked["one-hot"][1][0 * 25 + 3 * 5 + 2] == 0.0  # ln P(ATG) = -19 e^-60, about: 0 in the host's fp32
    return {name: (n.copy(), c.copy(), Entry(n, c)) for name, (n, c) in picked.items()}


@pytest.mark.parametrize("epsilon", [0.01, 0.1])
def test_it_is_the_model_of_emission_probs(entries, epsilon):
    e32 = np.float32(epsilon)
    for name, (nucltp, codonm, entry) in entries.items():
        want = emission_probs(float(e32), nucltp, codonm)[0]
        got = np.array([float(v) for v in entry.probs(e32)])
        assert np.array_equal(got == 0.0, want == 0.0), name
        assert (want > 0.0).sum() > 1000, name
        rel = np.abs(got - want)[want > 0.0] / want[want > 0.0]
        assert rel.max() <= 1e-12, (name, rel.max())


@pytest.mark.parametrize("epsilon", [1e-12, 1e-30])
def test_log_of_the_float64_probabilities_is_not_the_model(entries, epsilon):
    """Nobody compares a kernel's words against log(emission_probs) again: at P(ATG) ~ 1 it is more than 100 fp32
    ulps from ln P (measured: 204 at 1e-12; at 1e-30 it says ln 1 = 0, 1.1e7 ulps from -4e-30)."""
    e32 = np.float32(epsilon)
    nucltp, codonm, entry = entries["one-hot"]
    exact = float(entry.ln(e32)[ATG])
    assert -5 * float(e32) < exact < -3.9 * float(e32)
    f64 = np.log(emission_probs(float(e32), nucltp, codonm)[0, ATG])
    ulps = abs(f64 - exact) / exact_emission.ulp32(exact)
    print(f"epsilon {e32!r}: log(emission_probs) {f64!r}, exact {exact!r}, {ulps:.3g} fp32 ulps apart")
    assert ulps > 100
    assert kernel_formula(e32, nucltp, codonm)[ATG] == entry.rounded(e32).nearest[ATG]


@pytest.mark.parametrize("epsilon", EPSILONS + TIE_PRONE)
def test_the_kernel_formula_in_float64_gives_the_nearest_fp32(entries, epsilon):
    """'Rounded once': the formula of press_emission.h, evaluated in float64 and narrowed, is the correctly rounded
    fp32 of the exact ln P on every code of every entry -- not merely one of the two neighbours."""
    e32 = np.float32(epsilon)
    finite = 0
    for name, (nucltp, codonm, entry) in entries.items():
        got = kernel_formula(e32, nucltp, codonm)
        want = entry.rounded(e32)
        assert not np.isnan(got).any() and not np.isposinf(got).any(), name
        assert np.array_equal(np.isneginf(got), want.zero), name
        off = np.flatnonzero(~want.zero & (got != want.nearest))
        assert len(off) == 0, (f"{name} at epsilon {e32!r}: {len(off)} codes off the nearest fp32, first code {off[0]}: "
                               f"{got[off[0]]!r} for ln P = {want.lnp[off[0]]!r}")
        finite += int((~want.zero).sum())
    if epsilon in (0.0, 1.0):
        assert 0 < finite <= 5 * 64  # only whole codons (e = 0), only the four-error term of a 3-mer (e = 1)
    else:
        assert finite > 5 * 1000


def test_decimal_and_mpmath_agree(entries):
    """oracle/pydecode.py's statement of the model, run on mpmath numbers at 150 digits, against the decimal engine's
    ln P: 45 digits at least, on the entry and the error rates where the float64 form fails."""
    mpmath = pytest.importorskip("mpmath")
    from oracle import pydecode

    nucltp, codonm, entry = entries["one-hot"]
    with mpmath.workdps(150):
        def prob(v):
            return mpmath.mpf(0) if np.isneginf(v) else mpmath.exp(mpmath.mpf(float(v)))

        p = [prob(v) for v in nucltp]
        M = np.empty(125, object)
        M[:] = [prob(v) for v in codonm]
        M = M.reshape(5, 5, 5)
        for epsilon in (1e-30, 0.1):
            e = mpmath.mpf(float(np.float32(epsilon)))
            ours = entry.ln(np.float32(epsilon))
            for code, z in enumerate(exact_emission.code_digits()):
                P = pydecode.emission_prob(e, p, M, list(z))
                if ours[code] is None:
                    assert P == 0, code
                    continue
                want, got = mpmath.log(P), mpmath.mpf(str(ours[code]))
                assert abs(got - want) <= abs(want) * mpmath.mpf(10) ** -45, (epsilon, code, got, want)


def test_round_to_fp32_decides_in_decimal():
    """A value a hair above the midpoint of two fp32 neighbours, closer to it than float64 resolves: through float64
    it would be a tie and go to the even neighbour, below; straight from the decimal it goes up."""
    from decimal import Decimal

    below = np.float32(-1.5)
    assert int(below.view(np.uint32)) % 2 == 0
    above = np.nextafter(below, np.float32(0))
    mid = (Decimal(float(below)) + Decimal(float(above))) / 2
    x = exact_emission.WORK.add(mid, Decimal("1e-30"))
    assert np.float32(float(x)) == below  # the detour: float64 makes it the midpoint, fp32 ties to even
    lo, hi, nearest, rel = exact_emission.round_to_fp32(x)
    assert (lo, hi, nearest) == (below, above, above) and 0 < rel < 1e-29
    lo, hi, nearest, rel = exact_emission.round_to_fp32(exact_emission.WORK.subtract(mid, Decimal("1e-30")))
    assert (lo, hi, nearest) == (below, above, below)
    assert exact_emission.round_to_fp32(Decimal(float(below)))[:3] == (below, below, below)


def test_where_double_ends():
    """The domain of the kernels' formula.  A product of three inputs is taken in double
    before its log.  With every input at x nats it is e^3x: a normal double down to x = -236 (e^-708), where the
    formula still gives the nearest fp32; 0 from x = -249 on (e^-747, below the smallest subnormal e^-744.4), where
    the finite ln P of a 5-mer, ln(1/16) + 3x at e = 0.5, comes out -inf.  A 3-mer never takes the product (its ppp
    term is the sum of the inputs) and stays the nearest fp32."""
    for x, lost in ((-236.0, False), (-249.0, True)):
        nucltp, codonm = np.full(4, x, np.float32), np.full(125, x, np.float32)
        want = Entry(nucltp, codonm).rounded(0.5)
        got = kernel_formula(0.5, nucltp, codonm)
        assert not want.zero.any()
        assert np.allclose(want.lnp[340:], np.log(1 / 16) + 3 * x, rtol=1e-12)
        assert np.array_equal(got[20:84], want.nearest[20:84])
        if lost:
            assert np.isneginf(got[340:]).all()
        else:
            assert np.array_equal(got, want.nearest)
