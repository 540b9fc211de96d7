"""The yardstick of the ladder calibration's fit (dcp_hip_calibrate_lengths), in float64 numpy: one lambda per profile,
common to its rungs, by maximum likelihood with a location per rung, and the location of every rung at a lambda.
tests/test_calibrate_lengths_host.py holds it to known parameters; tests/test_gpu_calibrate_lengths.py holds the GPU to
it."""
import math

import numpy as np


def kept_of(x):
    """the finite scores of a rung, as float64"""
    x = np.asarray(x)
    return x[np.isfinite(x)].astype(np.float64)


def informative(rungs):
    """y = x - min x of the rungs that carry scale: at least two scores, not all equal"""
    ys = [x - x.min() for x in rungs if len(x) >= 2]
    return [y for y in ys if y.max() > 0]


def g_of(ys, lam):
    """g(lambda) = sum_j n_j (1 / lambda - mean_j y + T1_j / T0_j)"""
    total = 0.0
    for y in ys:
        e = np.exp(-lam * y)
        total += len(y) * (1.0 / lam - y.mean() + (y * e).sum() / e.sum())
    return total


def solve_lambda(rungs):
    """the root of g by bisection, 200 halvings of a bracket found by doubling; NaN without an informative rung"""
    ys = informative(rungs)
    if not ys:
        return math.nan
    lo = hi = 1.0
    while g_of(ys, lo) <= 0:
        lo /= 2
    while g_of(ys, hi) > 0:
        hi *= 2
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if g_of(ys, mid) > 0:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def mu_of(x, lam):
    """m - log(mean exp(-lambda (x - m))) / lambda over the kept scores of one rung; NaN for none"""
    if len(x) == 0 or math.isnan(lam):
        return math.nan
    m = x.min()
    return m - math.log(np.exp(-lam * (x - m)).mean()) / lam


def fit(scores, lam=None):
    """(lambda, [mu_j]) of a profile from its scores per rung (any float arrays; the non-finite are left out).  lam None:
    fitted."""
    rungs = [kept_of(x) for x in scores]
    if lam is None:
        lam = solve_lambda(rungs)
    return lam, [mu_of(x, lam) for x in rungs]
