"""The float64 numpy restatement of the FPFH contract (se3et_amd/fpfh.py, csrc/fpfh.hip, csrc/fpfh_core.h): the yardstick of
tests/test_fpfh_cpu.py and tests/test_gpu_fpfh.py.  Open3D is not a dependency of the tests; the contract is stated in the module docstring
of se3et_amd/fpfh.py and restated here operation by operation: vectorised over the pairs (numpy's +, -, *, /, sqrt round as the C operators
do), the FPFH sum loop-wise in the stated order (ascending neighbour index).

  search               brute force: d^2 = (dx dx + dy dy) + dz dz; radius: d^2 < r r; knn: the K first of np.lexsort on (d^2, index), the row
                       itself among them; hybrid: those of the K with d^2 < r r.  -> per row the members' indices, ascending.
  pair_features        f1, f2, x, y of every pair.
  bins                 the two linear bins and the sector rule.
  margins              per pair the distance to the nearest interior bin edge: |11 (f + 1) / 2 - nearest integer of 1..10| for f1 and f2, the
                       sector margin min_k |c_k y - s_k x| / (|x| + |y|) over the edges the rule tests, and the seam x < 0, 0 < |y| < 1e-9 |x|.
                       A pair within FLAG of an edge is flagged: its bin may legitimately differ between two correct implementations.
  spfh / fpfh          the two passes."""
import numpy as np

BINS, DIM = 11, 33
FLAG = 1e-9
# (cos, sin) of beta_k = -pi + 2 pi k / 11, k = 1 .. 10: the literals of csrc/fpfh_core.h
SECTORS = np.array([[-0.8412535328311812, -0.5406408174555976], [-0.41541501300188644, -0.9096319953545183],
                    [0.14231483827328514, -0.9898214418809327], [0.6548607339452851, -0.7557495743542583],
                    [0.9594929736144974, -0.28173255684142967], [0.9594929736144974, 0.28173255684142967],
                    [0.6548607339452851, 0.7557495743542583], [0.14231483827328514, 0.9898214418809327],
                    [-0.41541501300188644, 0.9096319953545183], [-0.8412535328311812, 0.5406408174555976]])


def _f64(a):
    return np.asarray(a).astype(np.float64).reshape(-1, 3)


def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)


def search(points, radius=None, max_nn=None):
    """-> list of int64 arrays: the members of every row's search result, ascending in index (the row itself among them where the search
    finds it)."""
    if radius is None and max_nn is None:
        raise ValueError('neither radius nor max_nn')
    p = _f64(points)
    index = np.arange(len(p))
    out = []
    for i in range(len(p)):
        d = p[i] - p
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        members = index
        if max_nn is not None:
            members = np.lexsort((index, d2))[:max_nn]
        if radius is not None:
            members = members[d2[members] < np.float64(radius) * np.float64(radius)]
        out.append(np.sort(members).astype(np.int64))
    return out


def pair_list(members):
    """-> (I, J) int64: every (row, neighbour) with the row itself dropped by index, rows ascending, neighbours ascending within a row"""
    I = np.concatenate([np.full(len(m) - int((m == i).sum()), i, np.int64) for i, m in enumerate(members)] + [np.zeros(0, np.int64)])
    J = np.concatenate([m[m != i] for i, m in enumerate(members)] + [np.zeros(0, np.int64)])
    return I, J


def pair_features(p1, n1, p2, n2):
    """-> (f1, f2, x, y) of M pairs; arrays (M, 3) float64"""
    with np.errstate(invalid='ignore', divide='ignore'):
        dp = p2 - p1
        d = np.sqrt(_dot(dp, dp))
        a1, a2 = _dot(n1, dp) / d, _dot(n2, dp) / d
        swap = np.abs(a1) < np.abs(a2)
        na, nb = np.where(swap[:, None], n2, n1), np.where(swap[:, None], n1, n2)
        dp = np.where(swap[:, None], -dp, dp)
        f2 = np.where(swap, -a2, a1)
        v = _cross(dp, na)
        length = np.sqrt(_dot(v, v))
        degenerate = (d == 0) | (length == 0)
        v = v / length[:, None]
        w = _cross(na, v)
        f1 = _dot(v, nb)
        x = _dot(na, nb)
        y = _dot(w, nb) + 0.0
    zero = np.zeros(len(d))
    return tuple(np.where(degenerate, zero, a) for a in (f1, f2, x, y))


def linear_bin(f):
    with np.errstate(invalid='ignore'):
        b = np.floor((11.0 * (f + 1.0)) * 0.5)
        return np.where(~(b >= 0), 0, np.where(b > 10, 10, b)).astype(np.int64)


def theta_bin(x, y):
    low = y < 0
    hits = (SECTORS[None, :, 0] * y[:, None] - SECTORS[None, :, 1] * x[:, None]) >= 0            # (M, 10): k = 1 .. 10
    b = np.where(low, hits[:, :5].sum(1), 5 + hits[:, 5:].sum(1))
    return np.where((x == 0) & (y == 0), 5, b).astype(np.int64)


def bins(f1, f2, x, y):
    """-> (theta bin, f1 bin, f2 bin)"""
    return theta_bin(x, y), linear_bin(f1), linear_bin(f2)


def margins(f1, f2, x, y):
    """-> (edge distance of f1, of f2, sector margin, seam flag, flagged)"""
    def edge(f):
        e = 11.0 * (f + 1.0) / 2.0
        return np.abs(e - np.clip(np.round(e), 1, 10))
    with np.errstate(invalid='ignore', divide='ignore'):
        low = y < 0
        dist = np.abs(SECTORS[None, :, 0] * y[:, None] - SECTORS[None, :, 1] * x[:, None]) / (np.abs(x) + np.abs(y))[:, None]
        sector = np.where(low, dist[:, :5].min(1), dist[:, 5:].min(1))
        sector = np.where((x == 0) & (y == 0), np.inf, sector)
    seam = (x < 0) & (np.abs(y) > 0) & (np.abs(y) < FLAG * np.abs(x))
    e1, e2 = edge(f1), edge(f2)
    return e1, e2, sector, seam, (e1 < FLAG) | (e2 < FLAG) | (sector < FLAG) | seam


def spfh(points, normals, members):
    """-> (counts (n, 33) int64, m (n,) int64, rows (n, 33) float64 = counts (100 / m), flagged (n,) bool: the row has a flagged pair)"""
    p, nr = _f64(points), _f64(normals)
    n = len(p)
    I, J = pair_list(members)
    f = pair_features(p[I], nr[I], p[J], nr[J])
    bt, b1, b2 = bins(*f)
    counts = np.zeros((n, DIM), np.int64)
    for off, b in ((0, bt), (BINS, b1), (2 * BINS, b2)):
        np.add.at(counts, (I, off + b), 1)
    m = np.bincount(I, minlength=n).astype(np.int64)
    with np.errstate(divide='ignore'):
        scale = np.where(m > 0, 100.0 / m.astype(np.float64), 0.0)
    flagged = np.zeros(n, bool)
    flagged[I[margins(*f)[4]]] = True
    return counts, m, counts.astype(np.float64) * scale[:, None], flagged


def fpfh(points, spfh_rows, members):
    """The second pass, loop-wise: every row adds its neighbours' terms in ascending neighbour index.  -> (n, 33) float64"""
    p = _f64(points)
    n = len(p)
    nbrs = [m[m != i] for i, m in enumerate(members)]
    width = max([len(b) for b in nbrs] + [0])
    table = np.full((n, width), -1, np.int64)
    for i, b in enumerate(nbrs):
        table[i, :len(b)] = b
    A = np.zeros((n, DIM))
    for t in range(width):
        rows = np.nonzero(table[:, t] >= 0)[0]
        j = table[rows, t]
        d = p[rows] - p[j]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        ok = d2 != 0
        A[rows[ok]] = A[rows[ok]] + spfh_rows[j[ok]] / d2[ok, None]
    F = np.empty((n, DIM))
    for g in range(3):
        S = np.zeros(n)
        for u in range(BINS):
            S = S + A[:, g * BINS + u]
        with np.errstate(divide='ignore', invalid='ignore'):
            scale = 100.0 / S
            for u in range(BINS):
                k = g * BINS + u
                F[:, k] = spfh_rows[:, k] + np.where(S != 0, A[:, k] * scale, A[:, k])
    return F


def compute(points, normals, radius=None, max_nn=None):
    """-> dict: members, counts, m, spfh, fpfh, flagged (the row has a flagged pair), tainted (the row or one of its neighbours has)"""
    members = search(points, radius, max_nn)
    counts, m, rows, flagged = spfh(points, normals, members)
    tainted = flagged.copy()
    for i, mem in enumerate(members):
        tainted[i] = tainted[i] or bool(flagged[mem].any())
    return {'members': members, 'counts': counts, 'm': m, 'spfh': rows, 'fpfh': fpfh(points, rows, members), 'flagged': flagged,
            'tainted': tainted}
