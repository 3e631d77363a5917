"""Independent float64 numpy twins of se3et_amd.segmentation (the contracts of csrc/plane.hip and csrc/dbscan.hip).

Plane: the sampler is se3et_amd.ransac.sample_indices, the fit numpy.linalg.eigh (or, as the second formulation that measures the twin's
own spread, a textbook cyclic Jacobi), the sums plain numpy sums (ascending, or descending for the spread).  DBSCAN: the literal
index-order sweep with a queue that Open3D and scikit-learn run, on brute-force neighbour lists."""
from collections import deque

import numpy as np

from se3et_amd.ransac import sample_indices

OK, TOO_FEW, NONE = 0, 2, 64


def _jacobi_smallest(C):
    a, v = C.copy(), np.eye(3)
    for _ in range(12):
        for p, q in ((0, 1), (0, 2), (1, 2)):
            if a[p, q] == 0.0:
                continue
            theta = 0.5 * np.arctan2(2.0 * a[p, q], a[q, q] - a[p, p])
            c, s = np.cos(theta), np.sin(theta)
            J = np.eye(3)
            J[p, p], J[q, q], J[p, q], J[q, p] = c, c, s, -s
            a, v = J.T @ a @ J, v @ J
    return v[:, int(np.argmin(np.diag(a)))], np.sort(np.diag(a))


def plane_of_rows(P, fit='eigh'):
    """The plane (a, b, c, d) of the rows P (m, 3) under item 3, or None where it is not defined; and the eigenvalue gap of the fit
    ((second smallest - smallest eigenvalue) / largest; inf for the cross product), which says how well the normal is defined."""
    P = np.asarray(P, np.float64)
    if len(P) < 3:
        return None, np.inf
    gap = np.inf
    with np.errstate(all='ignore'):
        if len(P) == 3:
            c, n = P[0], np.cross(P[1] - P[0], P[2] - P[0])
        else:
            c = P.mean(0)
            Q = P - c
            C = Q.T @ Q / len(P)
            if not C.any():
                return None, gap
            if not np.isfinite(C).all():
                return None, gap
            if fit == 'eigh':
                w, v = np.linalg.eigh(C)
                n = v[:, 0]
            else:
                n, w = _jacobi_smallest(C)
            gap = (w[1] - w[0]) / w[2] if w[2] > 0 else 0.0
        length = np.sqrt(n @ n)
        if not (length > 0 and np.isfinite(length)):
            return None, gap
        n = n / length
        lead = n[np.flatnonzero(n)[0]]
        if lead < 0:
            n = -n
        d = -(n @ c)
    if not np.isfinite(d):
        return None, gap
    return np.array([n[0], n[1], n[2], d]), gap


def _score(points, plane, thr, descending):
    dist = points @ plane[:3] + plane[3]
    inl = np.abs(dist) < thr
    sq = dist[inl] ** 2
    return dist, inl, float(np.sum(sq[::-1] if descending else sq))


def segment_plane(points, thr, ransac_n=3, num_iterations=100, seed=0, fit='eigh', descending=False):
    """The contract of csrc/plane.hip.  Returns a dict: plane, mask, count, fitness, inlier_rmse, status, best_hypothesis, hyp_counts, hyp_errs,
    and the facts the fixture asserts: margin (the smallest | |dist| - thr | over every evaluated hypothesis and the refit plane), gap (the
    smallest eigenvalue gap over the eigenvector fits), tie (the smallest relative difference of two error sums with equal counts that
    are not both exactly zero)."""
    points = np.asarray(points, np.float64).reshape(-1, 3)
    n, H = len(points), int(num_iterations)
    out = dict(plane=np.zeros(4), mask=np.zeros(n, bool), count=0, fitness=0.0, inlier_rmse=0.0, status=NONE, best_hypothesis=-1,
               hyp_counts=np.zeros(H, np.int64), hyp_errs=np.zeros(H), margin=np.inf, gap=np.inf, tie=np.inf)
    if n < ransac_n:
        out['status'] = TOO_FEW
        return out
    idx = sample_indices(seed, n, H, ransac_n)
    planes = []
    for h in range(H):
        plane, gap = plane_of_rows(points[idx[h]], fit)
        planes.append(plane)
        if plane is None:
            continue
        out['gap'] = min(out['gap'], gap)
        dist, inl, err = _score(points, plane, thr, descending)
        out['margin'] = min(out['margin'], float(np.min(np.abs(np.abs(dist) - thr))))
        out['hyp_counts'][h], out['hyp_errs'][h] = inl.sum(), err
    c, e = out['hyp_counts'], out['hyp_errs']
    for k in np.unique(c):
        errs = np.sort(e[c == k])
        for a, b in zip(errs[:-1], errs[1:]):
            if b > 0:
                out['tie'] = min(out['tie'], (b - a) / b)
    best = min(range(H), key=lambda h: (-c[h], e[h], h))
    if c[best] < 3:
        return out
    _, inl, _ = _score(points, planes[best], thr, descending)
    refit, gap = plane_of_rows(points[inl], fit)
    if refit is None:
        refit = planes[best]
    else:
        out['gap'] = min(out['gap'], gap)
    dist, inl, err = _score(points, refit, thr, descending)
    out['margin'] = min(out['margin'], float(np.min(np.abs(np.abs(dist) - thr))))
    count = int(inl.sum())
    out.update(plane=refit, mask=inl, count=count, fitness=count / n, inlier_rmse=float(np.sqrt(err / count)) if count else 0.0, status=OK,
               best_hypothesis=best)
    return out


def plane_spread(points, thr, ransac_n, num_iterations, seed):
    """The twin's own spread between two formulations (eigh and ascending sums against Jacobi and descending sums): the largest absolute
    difference of the plane coefficients, of fitness and of inlier_rmse.  The CPU tests allow 16 times this, and at least 1e-13."""
    a = segment_plane(points, thr, ransac_n, num_iterations, seed)
    b = segment_plane(points, thr, ransac_n, num_iterations, seed, fit='jacobi', descending=True)
    return dict(plane=float(np.max(np.abs(a['plane'] - b['plane']))), fitness=abs(a['fitness'] - b['fitness']),
                inlier_rmse=abs(a['inlier_rmse'] - b['inlier_rmse']))


def neighbours(points, eps):
    """The (n, n) bool relation of item 1: (dx dx + dy dy) + dz dz < eps eps, every operation rounded on its own."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    dx, dy, dz = (p[:, None, k] - p[None, :, k] for k in range(3))
    return (dx * dx + dy * dy) + dz * dz < eps * eps


def cluster_dbscan(points, eps, min_points):
    """The index-order sweep with breadth-first expansion: (labels (n,) int32, num_clusters)."""
    nb = neighbours(points, eps)
    n = len(nb)
    core = nb.sum(1) >= min_points
    labels = np.full(n, -1, np.int32)
    cluster = 0
    for i in range(n):
        if labels[i] != -1 or not core[i]:
            continue
        labels[i] = cluster
        queue = deque([i])
        while queue:
            u = queue.popleft()
            for v in np.flatnonzero(nb[u]):
                if labels[v] != -1:
                    continue
                labels[v] = cluster
                if core[v]:
                    queue.append(v)
        cluster += 1
    return labels, cluster


def eps_margin(points, eps):
    """The smallest | |p_i - p_j| - eps | / eps over all pairs: above 1e-9, d < eps and d <= eps are the same question."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    if len(p) < 2:
        return np.inf
    d = np.sqrt(sum((p[:, None, k] - p[None, :, k]) ** 2 for k in range(3)))
    return float(np.min(np.abs(d - eps))) / eps
