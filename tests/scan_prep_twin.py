"""The float64 numpy restatement of the scan-preparation contract (se3et_amd/scan_prep.py, csrc/voxel_downsample.hip, csrc/knn_normals.hip):
the yardstick of tests/test_scan_prep_cpu.py and tests/test_gpu_scan_prep.py.  Open3D is not a dependency of the tests; the contract is
stated in the module docstring of se3et_amd/scan_prep.py and restated here operation by operation.

  voxel_downsample     o = min - 0.5 v, i = floor((p - o) / v), voxels in the order of their first member, means by np.add.at (which adds
                       in ascending input index) and one division.
  knn                  brute force: d^2 = (dx dx + dy dy) + dz dz, each row ordered by np.lexsort on (d^2, index).
  covariances          sequential sums written as a loop over the list position.
  normals              np.linalg.eigh, the eigenvector of the smallest eigenvalue, canonical sign; (0, 0, 1) for m < 3 or C = 0.
  regularize_normals / modified_chamfer_distance   the reference's formulas in float64."""
import numpy as np

AXIS_CAP = float(2 ** 21)


def voxel_downsample(points, voxel_size, normals=None):
    """-> (means (m, 3), normal means or None, member counts (m,))"""
    p = np.asarray(points).astype(np.float64).reshape(-1, 3)
    nr = None if normals is None else np.asarray(normals).astype(np.float64).reshape(-1, 3)
    v = np.float64(voxel_size)
    if not (np.isfinite(v) and v > 0):
        raise ValueError('voxel size')
    if len(p) == 0:
        return np.zeros((0, 3)), (None if nr is None else np.zeros((0, 3))), np.zeros((0,), np.int64)
    if not np.isfinite(p).all() or (nr is not None and not np.isfinite(nr).all()):
        raise ValueError('non-finite point')
    o = p.min(0) - 0.5 * v
    if ((p.max(0) - o) / v >= AXIS_CAP).any():
        raise ValueError('too many voxels')
    i = np.floor((p - o) / v).astype(np.int64)
    key = i[:, 0] | (i[:, 1] << 21) | (i[:, 2] << 42)
    _, first, inverse, counts = np.unique(key, return_index=True, return_inverse=True, return_counts=True)
    order = np.argsort(first, kind='stable')                    # voxels by the input index of their first member
    rank = np.empty_like(order)
    rank[order] = np.arange(len(order))
    voxel = rank[inverse.reshape(-1)]
    counts = counts[order]

    def mean(a):
        s = np.zeros((len(order), 3))
        np.add.at(s, voxel, a)                                  # unbuffered: one addition per row, in ascending input index
        return s / counts[:, None].astype(np.float64)
    return mean(p), (None if nr is None else mean(nr)), counts


def knn(support, k, queries=None):
    """-> (idx (nq, k) int64, d2 (nq, k)): -1 / inf in the columns a small cloud leaves"""
    s = np.asarray(support).astype(np.float64).reshape(-1, 3)
    q = s if queries is None else np.asarray(queries).astype(np.float64).reshape(-1, 3)
    idx, d2 = np.full((len(q), k), -1, np.int64), np.full((len(q), k), np.inf)
    m = min(k, len(s))
    index = np.arange(len(s))
    for r in range(len(q)):
        d = q[r] - s
        row = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        best = np.lexsort((index, row))[:m]
        idx[r, :m], d2[r, :m] = best, row[best]
    return idx, d2


def covariances(points, idx):
    """Mean and covariance of every row's neighbours in list order.  -> (C (n, 6: xx xy xz yy yz zz), m)"""
    p = np.asarray(points).astype(np.float64).reshape(-1, 3)
    m = int((idx[0] >= 0).sum()) if len(idx) else 0
    nb = p[idx[:, :m]]                                          # (n, m, 3)
    s = np.zeros((len(idx), 3))
    for t in range(m):
        s = s + nb[:, t]
    with np.errstate(invalid='ignore', divide='ignore'):
        mean = s / np.float64(m)
        acc = np.zeros((len(idx), 6))
        for t in range(m):
            d = nb[:, t] - mean
            acc = acc + np.stack([d[:, 0] * d[:, 0], d[:, 0] * d[:, 1], d[:, 0] * d[:, 2], d[:, 1] * d[:, 1], d[:, 1] * d[:, 2],
                                  d[:, 2] * d[:, 2]], 1)
        return acc / np.float64(m), m


def full(C):
    return np.stack([C[:, [0, 1, 2]], C[:, [1, 3, 4]], C[:, [2, 4, 5]]], 1)


def canonical(n):
    n = n.copy()
    keep = (n[:, 2] > 0) | ((n[:, 2] == 0) & ((n[:, 1] > 0) | ((n[:, 1] == 0) & (n[:, 0] > 0))))
    n[~keep] = -n[~keep]
    return n


def normals_from(C, m):
    """-> (normals (n, 3), eigenvalues (n, 3) ascending)"""
    n = np.tile(np.array([0.0, 0.0, 1.0]), (len(C), 1))
    w = np.zeros((len(C), 3))
    solve = np.ones(len(C), bool) if m >= 3 else np.zeros(len(C), bool)
    solve &= (C != 0).any(1) if len(C) else solve
    if solve.any():
        ww, V = np.linalg.eigh(full(C[solve]))
        w[solve] = ww
        n[solve] = canonical(V[:, :, 0])
    return n, w


def estimate_normals(points, k=33, viewpoint=None):
    p = np.asarray(points).astype(np.float64).reshape(-1, 3)
    idx, _ = knn(p, k)
    C, m = covariances(p, idx)
    n, _ = normals_from(C, m)
    if viewpoint is not None:
        d = np.asarray(viewpoint, np.float64) - p
        flip = (n[:, 0] * d[:, 0] + n[:, 1] * d[:, 1]) + n[:, 2] * d[:, 2] < 0
        n[flip] = -n[flip]
    return n


def regularize_normals(points, normals, positive=True):
    """geotransformer/utils/pointcloud.py:25-37, literally"""
    dot_products = -(points * normals).sum(axis=1, keepdims=True)
    direction = dot_products > 0
    if positive:
        return normals * direction - normals * (1 - direction)
    return normals * (1 - direction) - normals * direction


def _nn_distance(q, s):
    return np.sqrt(knn(s, 1, q)[1][:, 0])


def _apply(T, p):
    return p @ T[:3, :3].T + T[:3, 3]


def modified_chamfer_distance(raw, ref, src, gt_transform, transform, reduction='mean'):
    """modules/registration/metrics.py:8-44 in float64, with exact nearest neighbours.  Arrays (B, N, 3) and (B, 4, 4)."""
    out = []
    for b in range(len(raw)):
        r, q, s = (np.asarray(a[b]).astype(np.float64) for a in (raw, ref, src))
        T, G = np.asarray(transform[b], np.float64), np.asarray(gt_transform[b], np.float64)
        out.append(_nn_distance(_apply(T, s), r).mean() + _nn_distance(q, _apply(T @ np.linalg.inv(G), r)).mean())
    out = np.array(out)
    return out.mean() if reduction == 'mean' else out.sum() if reduction == 'sum' else out
