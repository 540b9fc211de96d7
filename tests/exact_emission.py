"""The quasi-codon emission model in arbitrary precision, and the exact rounding of its
logarithms to fp32.  No product code: the standard library's decimal and numpy only.

An entry (a node, or the null or background model) is its fp32 log-probabilities as the kernels take them: nucltp[4]
and codonm[125], -inf meaning probability 0.  P(z) of each of the 1364 codes z is a sum of at most three terms
c e^a f^b poly(p, M), f = 1 - e, with the coefficients of oracle/pydecode.py: emission_prob.  The polynomials do not
depend on e: an Entry holds them, and an error rate then costs a few multiplications and one logarithm per code.

Precision.  Inputs, sums and products are taken with 130 digits, the logarithm with 55.  Every term is >= 0, so
nothing cancels and P carries a relative error of about 1e-129.  decimal's ln rounds correctly from the operand as
it stands, so ln P is off by 1e-129 absolute plus 1e-55 relative.  The smallest |ln P| that is not 0 comes from P
just below 1 and is of the order of the smallest fp32, 1.4e-45: the worst case is still good to 80 digits.

Rounding goes from the decimal value straight to fp32: the candidate a float64 detour names is only used to find
the two fp32 neighbours, and which of them is nearest is decided by comparing decimals."""
from __future__ import annotations

import decimal
import itertools
from dataclasses import dataclass
from decimal import Decimal

import numpy as np

TABLE_SIZE = 1364
ANY = 4
WORK = decimal.Context(prec=130, Emin=-999999, Emax=999999)  # inputs, polynomials, P
LOG = decimal.Context(prec=55, Emin=-999999, Emax=999999)  # ln P, correctly rounded from P as held
ZERO, ONE = Decimal(0), Decimal(1)


def exact(x) -> Decimal:
    """A binary floating-point value as the decimal it is, exactly."""
    return Decimal(float(x))


def prob(lprob) -> Decimal:
    """exp of an fp32 log-probability; -inf -> 0."""
    v = float(lprob)
    if v == float("-inf"):
        return ZERO
    if v != v or v == float("inf"):
        raise ValueError(f"not a log-probability: {v!r}")
    return WORK.exp(Decimal(v))


def code_digits():
    """The nucleotides of code 0, 1, ..: lengths 1..5 in turn, first nucleotide most significant."""
    for n in range(1, 6):
        yield from itertools.product(range(4), repeat=n)


def _sum(values) -> Decimal:
    total = ZERO
    for v in values:
        total = WORK.add(total, v)
    return total


def _mul(*values) -> Decimal:
    out = ONE
    for v in values:
        out = WORK.multiply(out, v)
    return out


@dataclass
class Rounded:
    """ln P of the 1364 codes of one entry at one error rate, between its fp32 neighbours."""

    zero: np.ndarray  # bool: P = 0 exactly; the other fields mean nothing there
    below: np.ndarray  # float32: the largest fp32 <= ln P
    above: np.ndarray  # float32: the smallest fp32 >= ln P (== below where ln P is an fp32)
    nearest: np.ndarray  # float32: the one of the two closer to ln P (ties to even)
    lnp: np.ndarray  # float64: ln P, for messages and bounds
    mid_rel: np.ndarray  # float64: |ln P - midpoint of the neighbours| / |ln P|; inf where ln P is an fp32

    @property
    def other(self) -> np.ndarray:
        """the neighbour that is not the nearest"""
        return np.where(self.nearest == self.below, self.above, self.below)


def round_to_fp32(x: Decimal):
    """-> (below, above, nearest, |x - midpoint| / |x|) of a finite decimal x within fp32's range."""
    c = np.float32(float(x))  # within one fp32 ulp of x: one of its neighbours
    if not np.isfinite(c):
        raise OverflowError(f"{x} is beyond fp32")
    dc = exact(c)
    if dc == x:
        return c, c, c, float("inf")
    if dc < x:
        below, above = c, np.nextafter(c, np.float32(np.inf))
    else:
        below, above = np.nextafter(c, np.float32(-np.inf)), c
    mid = WORK.divide(WORK.add(exact(below), exact(above)), Decimal(2))
    if x < mid:
        nearest = below
    elif x > mid:
        nearest = above
    else:  # an exact tie: the even mantissa
        nearest = below if int(below.view(np.uint32)) % 2 == 0 else above
    return below, above, nearest, float(WORK.divide(abs(WORK.subtract(x, mid)), abs(x)))


class Entry:
    """The polynomials of one entry: per code its terms (c poly, a, b) of c e^a (1 - e)^b poly(p, M)."""

    def __init__(self, nucltp, codonm):
        nucltp, codonm = np.asarray(nucltp, np.float32).reshape(4), np.asarray(codonm, np.float32).reshape(125)
        p = [prob(v) for v in nucltp]
        M = [prob(v) for v in codonm]

        def m(a, b, c):
            return M[a * 25 + b * 5 + c]

        def del1(a, b):  # codons with one base deleted that read (a, b)
            return _sum((m(ANY, a, b), m(a, ANY, b), m(a, b, ANY)))

        def one(a):  # codons holding a somewhere, two bases deleted
            return _sum((m(a, ANY, ANY), m(ANY, a, ANY), m(ANY, ANY, a)))

        def term(num, den, a, b, poly):
            return WORK.divide(WORK.multiply(Decimal(num), poly), Decimal(den)), a, b

        self.terms = []
        for z in code_digits():
            n = len(z)
            if n == 1:
                t = [term(1, 3, 2, 2, one(z[0]))]
            elif n == 2:
                t = [term(2, 3, 1, 3, del1(z[0], z[1])),
                     term(1, 3, 3, 1, _sum((_mul(p[z[0]], one(z[1])), _mul(p[z[1]], one(z[0])))))]
            elif n == 3:
                t = [term(1, 1, 0, 4, m(*z)),
                     term(4, 9, 2, 2, _sum((_mul(p[z[0]], del1(z[1], z[2])), _mul(p[z[1]], del1(z[0], z[2])),
                                            _mul(p[z[2]], del1(z[0], z[1]))))),
                     term(1, 1, 4, 0, _mul(p[z[0]], p[z[1]], p[z[2]]))]
            elif n == 4:  # one base inserted into a codon, or two inserted into a codon with one base deleted
                ins1 = _sum(_mul(p[z[j]], m(*(z[t] for t in range(4) if t != j))) for j in range(4))
                ins2 = _sum(_mul(p[z[i]], p[z[j]], del1(*(z[t] for t in range(4) if t not in (i, j))))
                            for i, j in itertools.combinations(range(4), 2))
                t = [term(1, 2, 1, 3, ins1), term(1, 9, 3, 1, ins2)]
            else:  # two bases inserted into a codon
                ins2 = _sum(_mul(p[z[i]], p[z[j]], m(*(z[t] for t in range(5) if t not in (i, j))))
                            for i, j in itertools.combinations(range(5), 2))
                t = [term(1, 10, 2, 2, ins2)]
            self.terms.append(t)
        assert len(self.terms) == TABLE_SIZE

    @staticmethod
    def _powers(epsilon):
        """e^0..e^4 and (1 - e)^0..(1 - e)^4 of the fp32 error rate; the zeroth power is 1 whatever e is"""
        e32 = np.float32(epsilon)
        if not 0.0 <= float(e32) <= 1.0:
            raise ValueError(f"error rate {epsilon!r}")
        e = exact(e32)
        f = WORK.subtract(ONE, e)
        E, F = [ONE], [ONE]
        for _ in range(4):
            E.append(WORK.multiply(E[-1], e))
            F.append(WORK.multiply(F[-1], f))
        return E, F

    def term_values(self, epsilon, code: int):
        """the terms of P(code) at the error rate, as probabilities"""
        E, F = self._powers(epsilon)
        return [_mul(cp, E[a], F[b]) for cp, a, b in self.terms[code]]

    def probs(self, epsilon):
        """P of every code: a list of 1364 decimals."""
        E, F = self._powers(epsilon)
        return [_sum(_mul(cp, E[a], F[b]) for cp, a, b in t) for t in self.terms]

    def largest_term(self, epsilon, code: int) -> float:
        """The largest |ln term| among the terms of P(code) that are not 0: the largest intermediate of a log-space
        evaluation.  0.0 when every term is 0."""
        return max((abs(float(LOG.ln(v))) for v in self.term_values(epsilon, code) if v != 0), default=0.0)

    def ln(self, epsilon):
        """ln P of every code as a 55-digit decimal, None where P = 0."""
        return [LOG.ln(v) if v != 0 else None for v in self.probs(epsilon)]

    def rounded(self, epsilon) -> Rounded:
        zero = np.zeros(TABLE_SIZE, bool)
        below, above, nearest = (np.zeros(TABLE_SIZE, np.float32) for _ in range(3))
        lnp, mid_rel = np.full(TABLE_SIZE, -np.inf), np.full(TABLE_SIZE, np.inf)
        for code, x in enumerate(self.ln(epsilon)):
            if x is None:
                zero[code] = True
            elif x == 0:  # P = 1 exactly
                lnp[code] = 0.0
            else:
                below[code], above[code], nearest[code], mid_rel[code] = round_to_fp32(x)
                lnp[code] = float(x)
        return Rounded(zero, below, above, nearest, lnp, mid_rel)


def ulp32(x) -> np.ndarray:
    """the spacing of fp32 at |x|, as float64"""
    a = np.abs(np.asarray(x, np.float64)).astype(np.float32)
    return (np.nextafter(a, np.float32(np.inf)).astype(np.float64) - a.astype(np.float64))
