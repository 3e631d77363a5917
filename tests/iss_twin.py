"""A numpy restatement of the ISS contract (se3et_amd/iss.py, csrc/iss.hip) for the tests: dense, one cloud, float64.

Memberships and counts use the contract's d^2 = (dx dx + dy dy) + dz dz and r r, so they are exact.  The scatter matrix is numpy's sum (any
order), the eigenvalues numpy.linalg.eigvalsh: both differ from the library's fixed-order sums and Jacobi sweeps by rounding, which the
tolerance below measures per cloud:

  E      the largest difference, relative to trace C, between eigvalsh of the float64 covariance and eigvalsh of the covariance formed in
         np.longdouble (rounded to float64 once): the arithmetic noise of the cloud's covariances.
  tol_i  16 max(E, 2^-53) trace C_i: what the library's eigenvalues of row i may differ by (16: the margin of the attention twin's rule).

An axis on which every member of a ball has the same coordinate gives an exactly zero row of C in any summation order (every deviation
from the mean is 0 when the mean is exact, which it is for equal values), and an eigenvalue that is exactly 0 in the library (a Jacobi
rotation never touches a zero row) and here (the axis is deflated before eigvalsh): such an eigenvalue is `exact`, and a decision between
exact operands is never flagged.

A row is flagged when one of its saliency decisions sits inside the tolerance: the two gamma tests, l3 > 0, and the comparison with a
member of its non_max_radius ball whose saliency differs from its own.  A row whose non_max_radius ball holds a flagged row is tainted."""
import numpy as np

U = 2.0 ** -53
MARGIN = 16.0


def dist2(p):
    """(n, n) d^2 by the contract's expression"""
    dx, dy, dz = (p[:, None, k] - p[None, :, k] for k in range(3))
    return (dx * dx + dy * dy) + dz * dz


def _covariances(p, members, dtype):
    """(n, 3, 3); a function of the member SET alone, so rows with the same members get the same bits (as they do in the library)"""
    q = p.astype(dtype)
    C = np.zeros((len(p), 3, 3), dtype)
    for i in range(len(p)):
        sel = q[members[i]]
        if len(sel):
            d = sel - sel.sum(0) / dtype(len(sel))
            C[i] = (d.T @ d) / dtype(len(sel))
    return C


def _eigenvalues(C):
    """(n, 3) descending, and which of them are exactly 0 by structure (a zero row of C)"""
    n = len(C)
    l, exact = np.zeros((n, 3)), np.zeros((n, 3), bool)
    for i in range(n):
        zero = ~C[i].any(1)
        live = np.flatnonzero(~zero)
        vals = np.linalg.eigvalsh(C[i][np.ix_(live, live)])[::-1] if len(live) else np.zeros(0)
        l[i, :len(vals)] = vals
        exact[i, len(vals):] = True
        if len(live) == 3:                                  # (no deflation: plain descending order)
            continue
        order = np.argsort(-l[i], kind='stable')            # a negative rounding residue sorts behind the exact zeros
        l[i], exact[i] = l[i][order], exact[i][order]
    return l, exact


def compute(points, salient_radius, non_max_radius, gamma_21=0.975, gamma_32=0.975, min_neighbors=5):
    p = np.asarray(points, np.float64).reshape(-1, 3)
    n = len(p)
    rs, rn = np.float64(salient_radius), np.float64(non_max_radius)
    d2 = dist2(p)
    members, near = d2 < rs * rs, d2 < rn * rn
    m, c = members.sum(1), near.sum(1)
    C = _covariances(p, members, np.float64)
    Cl = _covariances(p, members, np.longdouble).astype(np.float64)
    trace = np.trace(C, axis1=1, axis2=2)
    l, exact = _eigenvalues(C)
    ll, _ = _eigenvalues(Cl)
    live = trace > 0
    E = float((np.abs(l - ll).max(1)[live] / trace[live]).max()) if live.any() else 0.0
    tol = MARGIN * max(E, U) * trace
    nonzero = C.reshape(n, 9).any(1)
    with np.errstate(divide='ignore', invalid='ignore'):
        passes = (m >= min_neighbors) & nonzero & (l[:, 1] / l[:, 0] < gamma_21) & (l[:, 2] / l[:, 1] < gamma_32) & (l[:, 2] > 0)
    s = np.where(passes, l[:, 2], 0.0)
    # the decisions inside the tolerance (only where the earlier conditions leave them open)
    open_ = (m >= min_neighbors) & nonzero
    f21 = open_ & ~(exact[:, 0] & exact[:, 1]) & (np.abs(l[:, 1] - gamma_21 * l[:, 0]) <= tol * (1 + gamma_21))
    f32 = open_ & ~(exact[:, 1] & exact[:, 2]) & (np.abs(l[:, 2] - gamma_32 * l[:, 1]) <= tol * (1 + gamma_32))
    f0 = open_ & ~exact[:, 2] & (np.abs(l[:, 2]) <= tol)
    both = near & (s[:, None] > 0) & (s[None, :] > 0) & (s[:, None] != s[None, :])
    fnb = (both & (np.abs(s[:, None] - s[None, :]) <= tol[:, None] + tol[None, :])).any(1)
    flagged = f21 | f32 | f0 | fnb
    tainted = (near & flagged[None, :]).any(1)
    beaten = (near & (s[None, :] > s[:, None])).any(1)
    keypoint = (s > 0) & (c >= min_neighbors) & ~beaten
    return {'m': m, 'c': c, 'members': members, 'near': near, 'C': C, 'trace': trace, 'eigenvalues': l, 'exact': exact, 'E': E, 'tol': tol,
            'saliency': s, 'keypoint': keypoint, 'flagged': flagged, 'tainted': tainted}


def model_resolution(points):
    """(sum over the rows of the distance to the nearest other point) / n by math.fsum; 0 for n < 2"""
    import math
    p = np.asarray(points, np.float64).reshape(-1, 3)
    if len(p) < 2:
        return 0.0
    d2 = dist2(p)
    np.fill_diagonal(d2, np.inf)
    return math.fsum(np.sqrt(d2.min(1))) / len(p)
