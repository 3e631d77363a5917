"""An independent float64 twin of the weighted ICP contract (csrc/icp.hip, se3et_amd/icp.py: robust loss kernels and generalized ICP),
written from the contract and not from the library's text: scipy's cKDTree for the search, numpy.linalg.inv / solve / svd for the updates,
np.sin / np.cos for the rotation.  It keeps icp_twin.py's per-evaluation records: the correspondence of every source row and the two
margins under which the library must choose the same set."""
import numpy as np
from scipy.spatial import cKDTree

from icp_twin import SINGULAR, STEP_REFUSED, TOO_FEW, _evaluate, _vector6_to_matrix

LOSSES = ('l2', 'huber', 'cauchy', 'gm', 'tukey')
ESTIMATORS = ('point_to_point', 'point_to_plane', 'generalized')


def weight(loss, k, r):
    """Open3D's RobustKernel weights of the residuals r."""
    r = np.asarray(r, np.float64)
    a = np.abs(r)
    if loss == 'l2':
        return np.ones_like(r)
    if loss == 'huber':
        return np.where(a <= k, 1.0, k / np.maximum(a, k))
    if loss == 'cauchy':
        return 1.0 / (1.0 + (r / k) ** 2)
    if loss == 'gm':
        return k / (k + r ** 2) ** 2
    if loss == 'tukey':
        return np.where(a <= k, (1.0 - (r / k) ** 2) ** 2, 0.0)
    raise ValueError(loss)


def _skew(p):
    z = np.zeros(len(p))
    return np.stack([np.stack([z, -p[:, 2], p[:, 1]], 1), np.stack([p[:, 2], z, -p[:, 0]], 1), np.stack([-p[:, 1], p[:, 0], z], 1)], 1)


def _solve6(A, b):
    """(x, status): the 6x6 step, refused like the library's: not positive definite to rounding, or an angle of 1 rad."""
    w = np.linalg.eigvalsh(A)
    if not w[0] > 1e-12 * w[-1]:
        return None, SINGULAR
    x = np.linalg.solve(A, b)
    if np.abs(x[:3]).max() >= 1.0:
        return None, STEP_REFUSED
    return x, 0


def _weighted_kabsch(p, q, w):
    W = w.sum()
    pc, qc = (w[:, None] * p).sum(0) / W, (w[:, None] * q).sum(0) / W
    H = ((p - pc) * w[:, None]).T @ (q - qc)
    U, _s, Vt = np.linalg.svd(H)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))])
    R = Vt.T @ D @ U.T
    out = np.eye(4)
    out[:3, :3], out[:3, 3] = R, qc - R @ pc
    return out


def icp(src, ref, T0, r, mode='point_to_point', ref_normals=None, src_normals=None, loss='l2', loss_k=1.0, epsilon=1e-3,
        relative_fitness=1e-6, relative_rmse=1e-6, max_iteration=30):
    """-> dict(transform, fitness, fitness_ratio, rmse, iterations, converged, status, evaluations, condition: the largest condition number
    of the 6x6 systems it solved)."""
    src, ref, T = np.asarray(src, np.float64), np.asarray(ref, np.float64), np.array(T0, np.float64)
    nt_all = None if ref_normals is None else np.asarray(ref_normals, np.float64)
    ns_all = None if src_normals is None else np.asarray(src_normals, np.float64)
    assert len(src) and len(ref), 'the twin covers non-empty clouds'
    tree = cKDTree(ref)
    status, converged, evaluations, condition = 0, 0, [], 1.0
    rec, p, keep, j = _evaluate(tree, src, T, r)
    evaluations.append(rec)
    k = 0
    while k < max_iteration:
        U = np.eye(4)
        pk, qk = p[keep], ref[j[keep]]
        if mode == 'point_to_point':
            if rec['n_corr'] < 3:
                status |= TOO_FEW
            else:
                w = weight(loss, loss_k, np.sqrt(((pk - qk) ** 2).sum(1)))
                if not w.sum() > 0:
                    status |= SINGULAR
                else:
                    U = _weighted_kabsch(pk, qk, w)
        elif rec['n_corr'] < 6:
            status |= TOO_FEW
        else:
            if mode == 'point_to_plane':
                nk = nt_all[j[keep]]
                res = ((pk - qk) * nk).sum(1)
                J = np.concatenate([np.cross(pk, nk), nk], 1)
                w = weight(loss, loss_k, res)
                A, b = (J * w[:, None]).T @ J, -((J * w[:, None]).T @ res)
            else:
                nt, m = nt_all[j[keep]], ns_all[keep] @ T[:3, :3].T
                M = 2.0 * np.eye(3) - (1.0 - epsilon) * (nt[:, :, None] * nt[:, None, :] + m[:, :, None] * m[:, None, :])
                B = np.linalg.inv(M)
                d = pk - qk
                Am = np.concatenate([-_skew(pk), np.broadcast_to(np.eye(3), (len(pk), 3, 3))], 2)          # (n, 3, 6)
                w = weight(loss, loss_k, np.sqrt(np.einsum('na,nab,nb->n', d, B, d)))
                A = np.einsum('n,nra,nrs,nsb->ab', w, Am, B, Am)
                b = -np.einsum('n,nra,nrs,ns->a', w, Am, B, d)
            x, bad = _solve6(A, b)
            if x is not None:
                condition = max(condition, float(np.linalg.cond(A)))
            status |= bad
            if bad == STEP_REFUSED:
                break
            if x is not None:
                U = _vector6_to_matrix(x)
        T = U @ T
        k += 1
        prev = rec
        rec, p, keep, j = _evaluate(tree, src, T, r)
        evaluations.append(rec)
        if abs(rec['fitness'] - prev['fitness']) < relative_fitness and abs(rec['rmse'] - prev['rmse']) < relative_rmse:
            converged = 1
            break
    return {'transform': T, 'fitness': rec['fitness'], 'fitness_ratio': rec['fitness_ratio'], 'rmse': rec['rmse'], 'iterations': k,
            'converged': converged, 'status': status, 'evaluations': evaluations, 'condition': condition}
