"""Float64 numpy twin of se3et_amd/pair_geometry.py (csrc/pair_geometry.hip): the arithmetic contract restated by chunked brute force.

numpy only -- no scipy, no torch, no native code.  Every distance of every (query, support) pair is computed, so the twin has no search
structure that could be wrong in the way a grid can.
  moved point   fma(R[k][2], z, fma(R[k][1], y, R[k][0] * x)) + t[k]   (fma: Dekker's error-free product and Knuth's two-sum, which is the
                correctly rounded fma whenever the product is exact -- float32 inputs promoted -- and within one rounding of it otherwise)
  d^2           (dx dx + dy dy) + dz dz, every operation rounded;  tests d^2 < r r, strict; a nearest-neighbour distance is sqrt(d^2) and is
                tested as d d < r r
  nearest       np.argmin: the lowest index among equal d^2; an empty support gives inf / -1
  order         correspondences ascending in i, then j (np.nonzero's row-major order)
"""
import numpy as np

CHUNK = 1 << 22          # (query, support) pairs per block


def _two_prod(a, b):
    p = a * b
    ca, cb = 134217729.0 * a, 134217729.0 * b
    ah, bh = ca - (ca - a), cb - (cb - b)
    al, bl = a - ah, b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def fma(a, b, c):
    p, e = _two_prod(a, b)
    s = p + c
    bb = s - p
    t = (p - (s - bb)) + (c - bb)
    return s + (t + e)


def transform_points(points, transform):
    p = np.asarray(points, np.float64).reshape(-1, 3)
    if transform is None:
        return p.copy()
    T = np.asarray(transform, np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([fma(T[k, 2], z, fma(T[k, 1], y, T[k, 0] * x)) + T[k, 3] for k in range(3)], 1)


def _blocks(q, s):
    rows = max(1, CHUNK // max(1, len(s)))
    for a in range(0, len(q), rows):
        d = q[a:a + rows, None, :] - s[None, :, :]
        d *= d
        yield a, (d[:, :, 0] + d[:, :, 1]) + d[:, :, 2]


def scan(q_points, s_points, transform=None, radius=None):
    """(distances (nq,) float64, indices (nq,) int64, correspondences (n, 2) int64 or None without a radius): one pass over all pairs."""
    q = np.asarray(q_points, np.float64).reshape(-1, 3)
    s = transform_points(s_points, transform)
    dist, idx = np.full(len(q), np.inf), np.full(len(q), -1, np.int64)
    corr = []
    if len(s):
        for a, d2 in _blocks(q, s):
            j = np.argmin(d2, 1)
            idx[a:a + len(j)] = j
            dist[a:a + len(j)] = np.sqrt(d2[np.arange(len(j)), j])
            if radius is not None:
                i, jj = np.nonzero(d2 < radius * radius)
                corr.append(np.stack([i + a, jj], 1))
    if radius is None:
        return dist, idx, None
    return dist, idx, (np.concatenate(corr, 0) if corr else np.zeros((0, 2))).astype(np.int64).reshape(-1, 2)


def nearest_neighbor(q_points, s_points, transform=None):
    return scan(q_points, s_points, transform)[:2]


def overlap_from_distances(dist, radius):
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.float64(np.count_nonzero(dist * dist < radius * radius)) / np.float64(len(dist))


def compute_overlap(ref_points, src_points, transform, positive_radius):
    return overlap_from_distances(nearest_neighbor(ref_points, src_points, transform)[0], positive_radius)


def get_correspondences(ref_points, src_points, transform, matching_radius):
    return scan(ref_points, src_points, transform, matching_radius)[2]


def covariance_terms(points):
    """(sum G^T G, sum |terms|) over (n, 3) points, G = [I3 | -[p]x]; the second bounds the rounding of any summation order."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    out = []
    for q in (p, np.abs(p)):
        x, y, z = q[:, 0], q[:, 1], q[:, 2]
        n, absolute = float(len(q)), q is not p
        sg = 1.0 if absolute else -1.0
        C = np.zeros((6, 6))
        if len(q):
            C[0, 0] = C[1, 1] = C[2, 2] = n
            C[0, 4], C[0, 5] = z.sum(), sg * y.sum()
            C[1, 3], C[1, 5] = sg * z.sum(), x.sum()
            C[2, 3], C[2, 4] = y.sum(), sg * x.sum()
            C[3, 3], C[4, 4], C[5, 5] = (z * z + y * y).sum(), (z * z + x * x).sum(), (y * y + x * x).sum()
            C[3, 4], C[3, 5], C[4, 5] = sg * (x * y).sum(), sg * (x * z).sum(), sg * (y * z).sum()
            C = np.triu(C) + np.triu(C, 1).T
        out.append(C)
    return out[0], out[1]


def select_info_points(dist, idx, voxel_size, max_points=5000, seed=None):
    """The nearest-neighbour indices of the rows with d < voxel_size in row order; above max_points the reference's one draw on numpy's
    global generator (seeded first when a seed is given)."""
    sel = idx[dist * dist < voxel_size * voxel_size]
    if len(sel) > max_points:
        if seed is not None:
            np.random.seed(seed)
        sel = np.random.choice(sel, max_points, replace=False)
    return sel


def calibrate_ground_truth(ref_points, src_points, transform, voxel_size=0.006, max_points=5000, seed=None, nn=None):
    """(overlap at 5 voxel_size, covariance (6, 6), sum |terms| (6, 6), number of selected points)."""
    dist, idx = nearest_neighbor(ref_points, src_points, transform) if nn is None else nn
    sel = select_info_points(dist, idx, voxel_size, max_points, seed)
    cov, absolute = covariance_terms(transform_points(src_points, transform)[sel])
    return overlap_from_distances(dist, 5 * voxel_size), cov, absolute, len(sel)


def checksum(corr):
    """Order-sensitive 64-bit checksum of an (n, 2) correspondence list (wrapping uint64 arithmetic)."""
    c = np.asarray(corr, np.int64).reshape(-1, 2).astype(np.uint64)
    k = np.arange(len(c), dtype=np.uint64)
    with np.errstate(over='ignore'):
        return np.uint64(((c[:, 0] * np.uint64(1000003) + c[:, 1] + np.uint64(1)) * (np.uint64(2) * k + np.uint64(1))).sum(dtype=np.uint64))


# name -> (matching radius, overlap radii, voxel sizes): the cases of tests/golden/pair_geometry.npz
CASES = {
    'demo': (0.05, (0.0375, 0.1), (0.006, 0.025)),
    'c1_2k': (0.05, (0.0375,), (0.006, 0.025)),
    'c2_5k': (0.05, (0.0375,), (0.006, 0.025)),
    'c3_20k': (0.6, (0.45,), (0.3,)),
    'cap_30k': (0.05, (0.0375,), (0.006, 0.025)),
}


def case_inputs(name, index=0):
    """(ref, src, transform) float32 of a fixture case: the demo pair of tests/golden/demo_se3ete.npz, or a synthetic preset."""
    import os
    if name == 'demo':
        d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'demo_se3ete.npz'))
        return d['ref'], d['src'], d['transform']
    from se3et_amd.synthetic import make_pair
    return make_pair(name, index)
