"""An independent float64 twin of the coloured ICP contract (csrc/color_gradient.hip, csrc/icp.hip, se3et_amd/icp.py), written from the
contract and not from the library's text: an exhaustive distance table and numpy.linalg.lstsq for the gradients, and for the loop the
evaluation, the 6x6 solve, the update matrix and the loss weights of icp_twin / icp_robust_twin, by import."""
import numpy as np
from scipy.spatial import cKDTree

from icp_robust_twin import _solve6, weight
from icp_twin import STEP_REFUSED, TOO_FEW, _evaluate, _vector6_to_matrix


def intensity(colors):
    c = np.asarray(colors, np.float64)
    return (c[:, 0] + c[:, 1] + c[:, 2]) / 3.0


def gradients(points, normals, colors, radius, max_nn=30):
    """-> (gradients (n, 3), m (n,): the members of every row's search result, margins: the smallest |d^2 - r^2| of a listed entry and the
    smallest gap between the K-th and the (K + 1)-th d^2, under which the library must choose the same lists)."""
    p, nr, I = np.asarray(points, np.float64), np.asarray(normals, np.float64), intensity(colors)
    n = len(p)
    out, members = np.zeros((n, 3)), np.zeros(n, np.int64)
    radius_margin, tie_margin = np.inf, np.inf
    if n == 0:
        return out, members, (radius_margin, tie_margin)
    d = p[:, None, :] - p[None, :, :]
    d2 = d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1] + d[:, :, 2] * d[:, :, 2]
    r2 = float(radius) * float(radius)
    for i in range(n):
        order = np.lexsort((np.arange(n), d2[i]))
        near = order[:max_nn]
        if n > max_nn:
            tie_margin = min(tie_margin, d2[i, order[max_nn]] - d2[i, order[max_nn - 1]])
        radius_margin = min(radius_margin, np.abs(d2[i, near] - r2).min())
        member = near[d2[i, near] < r2]
        members[i] = m = len(member)
        if m < 4:
            continue
        nb = member[member != i]
        u = p[nb] - p[i]
        pr = u - (u @ nr[i])[:, None] * nr[i][None, :]
        A = np.concatenate([pr, (m - 1) * nr[i][None, :]], 0)
        b = np.concatenate([I[nb] - I[i], [0.0]])
        w = np.linalg.eigvalsh(A.T @ A)
        if not w[0] > 1e-12 * w[-1]:
            continue
        out[i] = np.linalg.lstsq(A, b, rcond=None)[0]
    return out, members, (float(radius_margin), float(tie_margin))


def icp(src, ref, T0, r, ref_normals, src_colors, ref_colors, ref_gradients, lambda_geometric=0.968, loss=None, loss_k=1.0,
        relative_fitness=1e-6, relative_rmse=1e-6, max_iteration=30):
    """-> dict(transform, fitness, fitness_ratio, rmse, iterations, converged, status, evaluations), as icp_twin.icp."""
    src, ref, T = np.asarray(src, np.float64), np.asarray(ref, np.float64), np.array(T0, np.float64)
    nt_all, g_all = np.asarray(ref_normals, np.float64), np.asarray(ref_gradients, np.float64)
    Is, It = intensity(src_colors), intensity(ref_colors)
    a, b = np.sqrt(lambda_geometric), np.sqrt(1.0 - lambda_geometric)
    assert len(src) and len(ref), 'the twin covers non-empty clouds'
    tree = cKDTree(ref)
    status, converged, evaluations = 0, 0, []
    rec, p, keep, j = _evaluate(tree, src, T, r)
    evaluations.append(rec)
    k = 0
    while k < max_iteration:
        U = np.eye(4)
        if rec['n_corr'] < 6:
            status |= TOO_FEW
        else:
            pk, jk = p[keep], j[keep]
            qk, nt, g = ref[jk], nt_all[jk], g_all[jk]
            s = ((pk - qk) * nt).sum(1)
            rg = a * s
            Jg = a * np.concatenate([np.cross(pk, nt), nt], 1)
            proj = (g * (pk - s[:, None] * nt - qk)).sum(1) + It[jk]
            rc = b * (Is[keep] - proj)
            d = -(g - (nt * g).sum(1)[:, None] * nt)
            Jc = b * np.concatenate([np.cross(pk, d), d], 1)
            wg = np.ones_like(rg) if loss is None else weight(loss, loss_k, rg)
            wc = np.ones_like(rc) if loss is None else weight(loss, loss_k, rc)
            A = (Jg * wg[:, None]).T @ Jg + (Jc * wc[:, None]).T @ Jc
            rhs = -((Jg * wg[:, None]).T @ rg + (Jc * wc[:, None]).T @ rc)
            x, bad = _solve6(A, rhs)
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
            'converged': converged, 'status': status, 'evaluations': evaluations}
