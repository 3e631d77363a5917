"""An independent float64 twin of the Fast Global Registration contract (csrc/fgr.hip, se3et_amd/fgr.py), written from the contract and
not from the library's text: numpy means and sums in numpy's order, numpy.linalg.solve for the 6x6 system, libm's sine and cosine, and
se3et_amd.ransac.sample_indices for the trials.  The tuple test's arithmetic -- (dx dx + dy dy) + dz dz and the two strict products -- is
elementwise and rounded operation by operation in numpy as in the library, so its decisions are the library's exactly; everything after it
differs from the library by rounding alone."""
import numpy as np

from se3et_amd.ransac import sample_indices

NONFINITE, TOO_FEW, SINGULAR, EMPTY, STEP_REFUSED, BAD_INDEX = 1, 2, 4, 8, 16, 32
MAX_ANGLE, MIN_CORRESPONDENCES, TRIALS_PER_CORRESPONDENCE, PIVOT_TOL = 4.0, 10, 100, 1e-13


def _edge2(points, i, j):
    d = points[i] - points[j]
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def tuple_test(S, R, C, tuple_scale, maximum_tuple_count, seed):
    """(C', the kept trials' indices) of item 1."""
    K = len(C)
    draws = sample_indices(seed, K, TRIALS_PER_CORRESPONDENCE * K, 3)
    tau2 = float(tuple_scale) * float(tuple_scale)
    ok = np.ones(len(draws), bool)
    for e in range(3):
        a, b = draws[:, e], draws[:, (e + 1) % 3]
        ls, lr = _edge2(S, C[a, 0], C[b, 0]), _edge2(R, C[a, 1], C[b, 1])
        ok &= (ls * tau2 < lr) & (lr * tau2 < ls)
    kept = np.nonzero(ok)[0][:maximum_tuple_count]
    return C[draws[kept].reshape(-1)], kept


def _positive_definite(A):
    """The solver's rule: every Cholesky pivot above PIVOT_TOL of its diagonal entry, and finite."""
    L = np.zeros((6, 6))
    for j in range(6):
        d = A[j, j] - (L[j, :j] ** 2).sum()
        if not (d > PIVOT_TOL * A[j, j]) or not np.isfinite(d):
            return False
        L[j, j] = np.sqrt(d)
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return True


def _update(x):
    cx, sx, cy, sy, cz, sz = np.cos(x[0]), np.sin(x[0]), np.cos(x[1]), np.sin(x[1]), np.cos(x[2]), np.sin(x[2])
    U = np.eye(4)
    U[:3, :3] = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ \
        np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    U[:3, 3] = x[3:]
    return U


def fgr(src, ref, corr, maximum_correspondence_distance=0.025, division_factor=1.4, use_absolute_scale=False, decrease_mu=True,
        iteration_number=64, tuple_scale=0.95, maximum_tuple_count=1000, tuple_test_on=True, seed=0):
    """-> dict(transform (4, 4), status, tuples (|C'|, 2), trials, mu, max_angle): the contract for one pair."""
    S, R = np.asarray(src, np.float64).reshape(-1, 3), np.asarray(ref, np.float64).reshape(-1, 3)
    C = np.asarray(corr, np.int64).reshape(-1, 2)
    out = {'transform': np.eye(4), 'status': 0, 'tuples': np.zeros((0, 2), np.int64), 'trials': np.zeros((0,), np.int64), 'mu': 0.0,
           'max_angle': 0.0}
    if not (np.isfinite(S).all() and np.isfinite(R).all()):
        out.update(status=NONFINITE, transform=np.full((4, 4), np.nan))
        return out
    if len(S) == 0 or len(R) == 0 or len(C) == 0:
        out['status'] = EMPTY
        return out
    if (C < 0).any() or (C[:, 0] >= len(S)).any() or (C[:, 1] >= len(R)).any():
        out.update(status=BAD_INDEX, transform=np.full((4, 4), np.nan))
        return out
    if tuple_test_on:
        C, out['trials'] = tuple_test(S, R, C, tuple_scale, maximum_tuple_count, seed)
    out['tuples'] = C
    if len(C) < MIN_CORRESPONDENCES:
        out['status'] = TOO_FEW
        return out
    mean_s, mean_r = S.mean(0), R.mean(0)
    scale = np.sqrt(max(((S - mean_s) ** 2).sum(1).max(), ((R - mean_r) ** 2).sum(1).max()))
    if not scale > 0:
        out['status'] = SINGULAR
        return out
    g, mu = (1.0, scale) if use_absolute_scale else (scale, 1.0)
    P, Q = (S[C[:, 0]] - mean_s) / g, (R[C[:, 1]] - mean_r) / g
    M = np.eye(4)
    for it in range(iteration_number):
        Qm = Q @ M[:3, :3].T + M[:3, 3]
        D = P - Qm
        w = (mu / ((D * D).sum(1) + mu)) ** 2
        A, b = np.zeros((6, 6)), np.zeros(6)
        for a in range(3):
            J = np.zeros((len(C), 6))
            J[:, 3 + a] = -1.0
            J[:, (a + 1) % 3] = -Qm[:, (a + 2) % 3]
            J[:, (a + 2) % 3] = Qm[:, (a + 1) % 3]
            A += (J * w[:, None]).T @ J
            b += (J * w[:, None]).T @ D[:, a]
        if not _positive_definite(A):
            out['status'] |= SINGULAR
        else:
            x = np.linalg.solve(A, -b)
            angle = np.abs(x[:3]).max() if np.isfinite(x[:3]).all() else np.inf
            out['max_angle'] = max(out['max_angle'], float(angle))
            if not angle < MAX_ANGLE:
                out['status'] |= STEP_REFUSED
                break
            M = _update(x) @ M
        if decrease_mu and it % 4 == 0 and mu > maximum_correspondence_distance:
            mu = mu / division_factor
    A = np.eye(4)
    A[:3, :3] = M[:3, :3]
    A[:3, 3] = -M[:3, :3] @ mean_r + g * M[:3, 3] + mean_s
    T = np.eye(4)
    T[:3, :3] = A[:3, :3].T
    T[:3, 3] = -A[:3, :3].T @ A[:3, 3]
    out.update(transform=T, mu=float(mu))
    return out
