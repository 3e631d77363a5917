"""The cases of the ISS tests (tests/test_iss_cpu.py, tests/test_gpu_iss.py), and the call of the library's host entry.

Clouds.
  patch        2000 points, default_rng(0), x, y uniform in [0, 1]^2, z = 0.5 + 0.12 sin(6x) cos(4y) + 0.05 x^2: a surface patch inside the
               unit box; salient_radius 0.08, non_max_radius 0.05.
  edge clouds  edge_clouds(): name -> (points, salient_radius, non_max_radius); gammas 0.975 and min_neighbors 5 throughout.
FACTS pins, per cloud, the ranges of the two member counts, the number of keypoints, the rows the twin flags or taints and the noise E of
tests/iss_twin.py as measured (the test allows twice that plus 2^-52: another BLAS sums in another order); the fixtures are chosen so
that the twin flags none.  A tight cluster's rows share one ball, hence one scatter matrix and one saliency: all of them are keypoints
(equal saliencies keep every row), which is what `clusters`, `copies` and `n5` count."""
import ctypes
import functools

import numpy as np

import iss_twin as twin

U = 2.0 ** -53
R_SALIENCY, R_SELECT = 4, 256          # rows per workgroup of iss_saliency_kernel (kIssWaves: one wave per row) and iss_select_kernel
MIN_NEIGHBORS = 5
PATCH_RADII = (0.08, 0.05)
CLUSTER_SIZES = (1, 2, 64, 65, 66, 301)          # rows with 0, 1, 63, 64, 65 and 300 members beside themselves

# cloud -> (least m, most m, least c, most c, keypoints, flagged or tainted rows, E as measured)
FACTS = {
    'patch': (10, 60, 4, 30, 75, 0, 1.1e-15),
    'clusters': (1, 301, 1, 301, 496, 0, 8.0e-16),
    'exact': (2, 2, 1, 2, 0, 0, 0.0),
    'min_neighbors': (4, 8, 1, 5, 10, 0, 9.4e-17),
    'planar': (40, 40, 40, 40, 0, 0, 0.0),
    'collinear': (12, 12, 12, 12, 0, 0, 1.5e-16),
    'copies': (8, 8, 16, 16, 16, 0, 0.0),
    'n0': (0, 0, 0, 0, 0, 0, 0.0), 'n1': (1, 1, 1, 1, 0, 0, 0.0), 'n2': (2, 2, 2, 2, 0, 0, 0.0), 'n3': (3, 3, 3, 3, 0, 0, 2.7e-16),
    'n4': (4, 4, 4, 4, 0, 0, 8.8e-17), 'n5': (5, 5, 5, 5, 5, 0, 5.2e-17),
    'n255': (2, 27, 1, 12, 10, 0, 7.0e-16), 'n256': (2, 29, 1, 13, 11, 0, 4.9e-16), 'n257': (2, 33, 1, 12, 16, 0, 1.1e-15),
}


def patch(n, seed):
    g = np.random.default_rng(seed)
    xy = g.uniform(0.0, 1.0, (n, 2))
    x, y = xy[:, 0], xy[:, 1]
    return np.stack([x, y, 0.5 + 0.12 * np.sin(6 * x) * np.cos(4 * y) + 0.05 * x * x], 1)


@functools.lru_cache(None)
def edge_clouds():
    """name -> (points, salient_radius, non_max_radius)"""
    g = np.random.default_rng(7)
    out = {'patch': (patch(2000, 0),) + PATCH_RADII}
    # tight clusters far apart: every row of a cluster of s points has s members at both radii (the tile of 64 of the saliency kernel)
    p = np.concatenate([10.0 * k + g.uniform(0, 0.1, (s, 3)) for k, s in enumerate(CLUSTER_SIZES)])
    out['clusters'] = (p[g.permutation(len(p))], 0.25, 0.2)
    # exact by construction: row 1 at exactly the salient radius of row 0 (0.25^2 = 0.0625: not a member), row 2 its duplicate (a member
    # of row 1), row 3 at exactly the non_max radius of row 0
    out['exact'] = (np.array([[0.0, 0, 0], [0.25, 0, 0], [0.25, 0, 0], [0, 0.125, 0]]), 0.25, 0.125)
    # min_neighbors - 1 and min_neighbors members, at each radius: tight groups (within 0.02) of 4 and of 5 points alone, and the same
    # groups with three satellites between the two radii (0.1 < d < 0.3, at three different distances: the scatter
    # matrix is anisotropic) that are no members of each other's non_max ball
    sat = np.array([[0.2, 0, 0], [0, 0.15, 0], [0.05, 0.05, 0.14]])
    groups = [g.uniform(0, 0.02, (4, 3)), g.uniform(0, 0.02, (5, 3)), np.concatenate([g.uniform(0, 0.02, (4, 3)), sat]),
              np.concatenate([g.uniform(0, 0.02, (5, 3)), sat])]
    out['min_neighbors'] = (np.concatenate([5.0 * k + q for k, q in enumerate(groups)]), 0.3, 0.1)
    # a planar cluster (z constant: l3 = 0 exactly) and a collinear one (y and z constant: l2 = l3 = 0): saliency 0
    flat = g.uniform(0, 0.1, (40, 3))
    flat[:, 2] = 0.375
    out['planar'] = (flat, 0.25, 0.2)
    line = np.zeros((12, 3))
    line[:, 0], line[:, 1], line[:, 2] = g.uniform(0, 0.1, 12), -0.25, 0.5
    out['collinear'] = (line, 0.25, 0.2)
    # two copies of one cluster on dyadic coordinates (multiples of 1 / 64 in [0, 1/8]: every sum of the contract is exact), 0.5 apart:
    # outside each other's salient balls (0.25), inside each other's non_max balls (1.0): bit-equal saliencies, every row kept
    one = g.integers(0, 9, (8, 3)).astype(np.float64) / 64.0
    out['copies'] = (np.concatenate([one, one + np.array([0.5, 0, 0])]), 0.25, 1.0)
    for n in (0, 1, 2, R_SALIENCY - 1, R_SALIENCY, R_SALIENCY + 1):
        out['n%d' % n] = (g.uniform(0, 0.1, (n, 3)), 0.25, 0.2)
    for n in (R_SELECT - 1, R_SELECT, R_SELECT + 1):
        out['n%d' % n] = (g.uniform(0, 1, (n, 3)), 0.25, 0.15)
    for v in out.values():
        v[0].setflags(write=False)
    return out


@functools.lru_cache(None)
def reference(name):
    """The twin's result of a named cloud, once."""
    p, rs, rn = edge_clouds()[name]
    return twin.compute(p, rs, rn, min_neighbors=MIN_NEIGHBORS)


def facts(name):
    r = reference(name)
    m, c = r['m'], r['c']
    lo = lambda a: int(a.min()) if len(a) else 0
    hi = lambda a: int(a.max()) if len(a) else 0
    return (lo(m), hi(m), lo(c), hi(c), int(r['keypoint'].sum()), int((r['flagged'] | r['tainted']).sum()), r['E'])


# ---- the library's host entry (the __host__ __device__ text of the kernels, no GPU) --------------------------------------------------------------
def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def host_iss(points, salient_radius, non_max_radius, gamma_21=0.975, gamma_32=0.975, min_neighbors=MIN_NEIGHBORS):
    """se3_debug_iss_host: {'saliency' (n,), 'eigenvalues' (n, 3), 'm' (n,), 'c' (n,), 'keypoint' (n,) bool, 'status'}"""
    from se3et_amd import _lib as L
    p = np.ascontiguousarray(points).reshape(-1, 3)
    assert p.dtype in (np.float32, np.float64)
    n = len(p)
    sal, eig, counts, mask = np.full(max(n, 1), -7.0), np.full((max(n, 1), 3), -7.0), np.full((max(n, 1), 2), -7, np.int64), np.full(max(n, 1), 7, np.uint8)
    status = np.full(1, -1, np.int32)
    L.check(L.lib().se3_debug_iss_host(_ptr(p if n else np.zeros((1, 3), p.dtype)), n, int(p.dtype == np.float64), float(salient_radius),
                                       float(non_max_radius), float(gamma_21), float(gamma_32), int(min_neighbors), _ptr(sal), _ptr(eig), _ptr(counts),
                                       _ptr(mask), _ptr(status)), 'se3_debug_iss_host')
    return {'saliency': sal[:n], 'eigenvalues': eig[:n], 'm': counts[:n, 0], 'c': counts[:n, 1], 'keypoint': mask[:n].astype(bool),
            'status': int(status[0])}


def host_resolution(points):
    """The model resolution of one cloud from se3_debug_knn_distance_host (k = 2, column 1) and se3_debug_distance_stats_host."""
    from se3et_amd import _lib as L
    p = np.ascontiguousarray(points).reshape(-1, 3)
    n = len(p)
    a, stats = np.zeros(max(n, 1)), np.zeros(4)
    L.check(L.lib().se3_debug_knn_distance_host(_ptr(p if n else np.zeros((1, 3), p.dtype)), n, int(p.dtype == np.float64), 2, 1, _ptr(a)),
            'se3_debug_knn_distance_host')
    L.check(L.lib().se3_debug_distance_stats_host(_ptr(a), n, 1.0, _ptr(stats), None), 'se3_debug_distance_stats_host')
    return float(stats[3])
