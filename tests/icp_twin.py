"""An independent float64 twin of the ICP contract (csrc/icp.hip, se3et_amd/icp.py), written from the contract and not from the library's
text: scipy's cKDTree for the search, numpy.linalg.svd / solve for the updates, np.sin / np.cos for the rotation.  Besides the result it
records, per evaluation, the correspondence of every source row and the two margins under which the library must choose the same set:
the distance of the nearest d to the threshold r, and the gap between a row's nearest and second-nearest reference point."""
import numpy as np
from scipy.spatial import cKDTree

NONFINITE, TOO_FEW, SINGULAR, EMPTY, STEP_REFUSED = 1, 2, 4, 8, 16


def _evaluate(tree, src, T, r, workers=1):
    p = src @ T[:3, :3].T + T[:3, 3]
    k = min(2, tree.n)
    d, j = tree.query(p, k=k, workers=workers)
    d, j = d.reshape(len(p), k), j.reshape(len(p), k)
    near = d[:, 0]
    keep = near < r
    corr = np.where(keep, j[:, 0], -1).astype(np.int64)
    n = int(keep.sum())
    rec = {'corr': corr, 'n_corr': n, 'fitness_ratio': (n, len(src)), 'fitness': n / len(src) if len(src) else 0.0,
           'rmse': float(np.sqrt((near[keep] ** 2).sum() / n)) if n else 0.0,
           'threshold_margin': float(np.abs(near - r).min()) if len(src) else np.inf,
           'gap_margin': float((d[:, 1] - d[:, 0]).min()) if k == 2 and len(src) else np.inf}
    return rec, p, keep, j[:, 0]


def _kabsch(p, q):
    pc, qc = p.mean(0), q.mean(0)
    H = (p - pc).T @ (q - qc)
    U, _s, Vt = np.linalg.svd(H)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))])
    R = Vt.T @ D @ U.T
    out = np.eye(4)
    out[:3, :3], out[:3, 3] = R, qc - R @ pc
    return out


def _vector6_to_matrix(x):
    sx, cx, sy, cy, sz, cz = np.sin(x[0]), np.cos(x[0]), np.sin(x[1]), np.cos(x[1]), np.sin(x[2]), np.cos(x[2])
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    out = np.eye(4)
    out[:3, :3], out[:3, 3] = Rz @ Ry @ Rx, x[3:]
    return out


def icp(src, ref, T0, r, mode='point_to_point', normals=None, relative_fitness=1e-6, relative_rmse=1e-6, max_iteration=30, workers=1):
    """-> dict(transform, fitness, fitness_ratio, rmse, iterations, converged, status, evaluations: the list of per-evaluation records).
    workers: the threads of the tree query (tools/icp_probe.py times the twin with 16)."""
    src, ref, T = np.asarray(src, np.float64), np.asarray(ref, np.float64), np.array(T0, np.float64)
    assert len(src) and len(ref), 'the twin covers non-empty clouds'
    tree = cKDTree(ref)
    status, converged, evaluations = 0, 0, []
    rec, p, keep, j = _evaluate(tree, src, T, r, workers)
    evaluations.append(rec)
    k = 0
    while k < max_iteration:
        U = np.eye(4)
        if mode == 'point_to_point':
            if rec['n_corr'] < 3:
                status |= TOO_FEW
            else:
                U = _kabsch(p[keep], ref[j[keep]])
        else:
            if rec['n_corr'] < 6:
                status |= TOO_FEW
            else:
                pk, qk, nk = p[keep], ref[j[keep]], np.asarray(normals, np.float64)[j[keep]]
                res = ((pk - qk) * nk).sum(1)
                J = np.concatenate([np.cross(pk, nk), nk], 1)
                A, b = J.T @ J, -(J.T @ res)
                w = np.linalg.eigvalsh(A)
                if not w[0] > 1e-12 * w[-1]:
                    status |= SINGULAR
                else:
                    x = np.linalg.solve(A, b)
                    if np.abs(x[:3]).max() >= 1.0:
                        status |= STEP_REFUSED
                        break
                    U = _vector6_to_matrix(x)
        T = U @ T
        k += 1
        prev = rec
        rec, p, keep, j = _evaluate(tree, src, T, r, workers)
        evaluations.append(rec)
        if abs(rec['fitness'] - prev['fitness']) < relative_fitness and abs(rec['rmse'] - prev['rmse']) < relative_rmse:
            converged = 1
            break
    return {'transform': T, 'fitness': rec['fitness'], 'fitness_ratio': rec['fitness_ratio'], 'rmse': rec['rmse'], 'iterations': k,
            'converged': converged, 'status': status, 'evaluations': evaluations}
