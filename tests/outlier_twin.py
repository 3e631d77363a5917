"""A numpy restatement of the outlier-removal contract (se3et_amd/scan_prep.py, csrc/outliers.hip) for the tests: dense, one cloud, float64.

The k-NN list is the contract's ((d^2, index) ascending, d^2 = (dx dx + dy dy) + dz dz, the row itself included) and the row value a_i is
its sequential sum of correctly rounded roots, so a_i is exact.  The two cloud sums are math.fsum's: the library's fixed-shape sums of
non-negative terms agree with them to (n + 16) 2^-53 relative (n additions of at most 2^-53 each, and the few roundings of the mean, the
division, the root and the threshold), which is the tolerance on mean, std and thr.  A row is flagged when
|a_i - thr| <= 2 (n + 16) 2^-53 thr.  Two kinds of row are decided exactly and never flagged: a row with a_i <= 0 (dropped by the exact
test a_i > 0, whatever thr is), and the rows of a two-point cloud (a_0 = a_1 = d / 2; their sum 2 a and its half are exact in either
order, so mean = a, std = 0 and thr = a on both sides: a < thr is false on both)."""
import math

import numpy as np

from iss_twin import dist2

U = 2.0 ** -53


def row_means(points, nb_neighbors):
    p = np.asarray(points, np.float64).reshape(-1, 3)
    n = len(p)
    m = min(int(nb_neighbors), n)
    if n == 0:
        return np.zeros(0)
    d2 = dist2(p)
    order = np.lexsort((np.broadcast_to(np.arange(n), (n, n)), d2), axis=1)[:, :m]          # (d^2, index) ascending
    roots = np.sqrt(np.take_along_axis(d2, order, 1))
    s = np.zeros(n)
    for t in range(m):
        s = s + roots[:, t]
    return s / float(m)


def statistics(a, std_ratio):
    """(mean, std, thr) with fsum; NaN where the formulas give NaN"""
    n = len(a)
    pos = a[a > 0]
    with np.errstate(divide='ignore', invalid='ignore'):                # (n = 0: 0 / 0 and 0 / -1; n = 1: 0 / 0, as the formulas give)
        mean = np.float64(math.fsum(pos)) / np.float64(n)
        std = np.sqrt(np.float64(math.fsum((pos - mean) ** 2)) / np.float64(n - 1))
        return float(mean), float(std), float(mean + np.float64(std_ratio) * std)


def statistical(points, nb_neighbors=20, std_ratio=2.0):
    a = row_means(points, nb_neighbors)
    n = len(a)
    mean, std, thr = statistics(a, std_ratio)
    with np.errstate(invalid='ignore'):
        keep = (a > 0) & (a < thr)
        flagged = (a > 0) & (np.abs(a - thr) <= 2 * (n + 16) * U * thr) & (n != 2)
    return {'a': a, 'mean': mean, 'std': std, 'thr': thr, 'keep': keep, 'flagged': flagged, 'tolerance': (n + 16) * U}


def radius(points, nb_points, r):
    p = np.asarray(points, np.float64).reshape(-1, 3)
    r = np.float64(r)
    counts = (dist2(p) < r * r).sum(1) if len(p) else np.zeros(0, np.int64)
    return {'counts': counts, 'keep': counts > nb_points}
