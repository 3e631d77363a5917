"""The cases of the FPFH tests (tests/test_fpfh_cpu.py, tests/test_gpu_fpfh.py), and the call of the library's host entry.

Clouds.
  surface      1500 points, default_rng(0), x, y uniform in [-1, 1]^2, z = 0.3 sin(3x) cos(2y) + 0.1 x^2 with analytic unit normals; radius
               0.25 gives a mean of 59.7 neighbours.  Asymmetric on purpose: a box matches itself under its symmetries.
  micro, c1_2k the clouds of tests/scan_prep_fixture.py with the normals of its twin (k = 33).
  edge clouds  two-point clouds whose pair is exact by construction from axis-aligned values (PAIR_EDGES: the bins of row 0 are pinned as
               literals), and the degenerate rows and neighbour counts of edge_clouds().
FACTS pins, per case, the range of the neighbour counts and the number of pairs the twin flags (test_fixture_facts); the fixtures are
chosen so that it flags none."""
import ctypes
import functools

import numpy as np

import fpfh_twin as twin
import scan_prep_fixture as S

U = 2.0 ** -53
R = 4                         # rows per workgroup of spfh_kernel and of fpfh_kernel (kFpfhWaves, csrc/fpfh.hip): one wave per row
MOTION_ROTVEC, MOTION_SHIFT = (0.4, -0.7, 1.1), (0.3, -1.2, 0.5)

# case -> (cloud, radius, max_nn)
CASES = {'surface_radius': ('surface', 0.25, None), 'surface_knn': ('surface', None, 33), 'surface_hybrid': ('surface', 0.2, 48),
         'micro_radius': ('micro', 0.12, None), 'c1_2k_radius': ('c1_2k', 0.25, None), 'c1_2k_hybrid': ('c1_2k', 0.2, 64)}
# case -> (least neighbours, most neighbours, flagged pairs)
FACTS = {'surface_radius': (15, 94, 0), 'surface_knn': (32, 32, 0), 'surface_hybrid': (10, 47, 0), 'micro_radius': (9, 32, 0),
         'c1_2k_radius': (38, 109, 0), 'c1_2k_hybrid': (22, 63, 0)}
EDGE_FACTS = {'clusters': (0, 300, 0), 'dense': (199, 199, 0), 'isolated': (0, 0, 0), 'one_neighbour': (0, 1, 0), 'knn_1': (0, 0, 0),
              'knn_2': (1, 1, 0), 'knn_64': (63, 63, 0), 'knn_above_n': (8, 8, 0), 'hybrid': (1, 19, 0), 'duplicates': (2, 19, 0),
              'duplicates_knn': (63, 64, 0), 'n0': (0, 0, 0), 'n1': (0, 0, 0), 'n2': (0, 0, 0), 'n3': (0, 1, 0), 'n4': (2, 3, 0), 'n5': (3, 4, 0)}


def surface(n, seed):
    """n points of z = 0.3 sin(3x) cos(2y) + 0.1 x^2 over [-1, 1]^2 with their analytic unit normals"""
    g = np.random.default_rng(seed)
    xy = g.uniform(-1.0, 1.0, (n, 2))
    x, y = xy[:, 0], xy[:, 1]
    z = 0.3 * np.sin(3 * x) * np.cos(2 * y) + 0.1 * x * x
    zx = 0.9 * np.cos(3 * x) * np.cos(2 * y) + 0.2 * x
    zy = -0.6 * np.sin(3 * x) * np.sin(2 * y)
    nr = np.stack([-zx, -zy, np.ones_like(x)], 1)
    return np.stack([x, y, z], 1), nr / np.linalg.norm(nr, axis=1, keepdims=True)


@functools.lru_cache(None)
def cloud(name):
    """-> (points (n, 3) float64, normals (n, 3) float64)"""
    out = surface(1500, 0) if name == 'surface' else (S.cloud(name).astype(np.float64), S.twin_normals(name)[2].copy())
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(None)
def reference(case):
    """The twin's result of a named case, once."""
    name, radius, max_nn = CASES[case]
    return twin.compute(*cloud(name), radius, max_nn)


def facts(points, normals, radius, max_nn, result=None):
    """-> (least neighbours, most neighbours, pairs the twin flags) of a cloud"""
    r = result or twin.compute(points, normals, radius, max_nn)
    p, nr = np.asarray(points, np.float64).reshape(-1, 3), np.asarray(normals, np.float64).reshape(-1, 3)
    I, J = twin.pair_list(r['members'])
    flagged = twin.margins(*twin.pair_features(p[I], nr[I], p[J], nr[J]))[4]
    m = r['m']
    return (int(m.min()) if len(m) else 0, int(m.max()) if len(m) else 0, int(flagged.sum()))


def rotation(rotvec):
    v = np.asarray(rotvec, np.float64)
    angle = np.linalg.norm(v)
    k = v / angle
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def moved_surface():
    """-> (points, normals, permutation, R, t): the surface cloud rotated, translated and permuted; moved row k is original row perm[k]"""
    p, nr = cloud('surface')
    Rm, t = rotation(MOTION_ROTVEC), np.asarray(MOTION_SHIFT)
    perm = np.random.default_rng(5).permutation(len(p))
    return (p @ Rm.T + t)[perm], (nr @ Rm.T)[perm], perm, Rm, t


# name -> (p1, n1, p2, n2, (theta, f1, f2) bins of the pair (p1, p2)): exact by construction; radius 2 holds both points
PAIR_EDGES = {
    'duplicate': ((0, 0, 0), (0, 0, 1), (0, 0, 0), (1, 0, 0), (5, 5, 5)),                      # d == 0: degenerate, counted
    'dp_parallel_n1': ((0, 0, 0), (0, 0, 1), (0, 0, 1), (1, 0, 0), (5, 5, 5)),                 # v = dp x n1 = 0
    'equal_angles': ((0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (8, 5, 9)),                   # |a1| == |a2|: no swap (a swap gives f2 bin 1)
    'swap': ((0, 0, 0), (0, 1, 0), (1, 0.5, 0), (1, 0, 0), (2, 5, 0)),                         # |a1| < |a2|: swapped (none gives f2 bin 7)
    'f1_plus_one': ((0, 0, 0), (0, 0, 1), (1, 0, 0), (0, -1, 0), (5, 10, 5)),                  # f1 == 1: bin 10 by the clamp; x == y == 0
    'f1_minus_one': ((0, 0, 0), (0, 0, 1), (1, 0, 0), (0, 1, 0), (5, 0, 5)),                   # f1 == -1, x == y == 0: theta bin 5
    'opposite_normals': ((0, 0, 0), (0, 0, 1), (1, 0, 0), (-0.0, -0.0, -1), (10, 5, 5)),       # n1 . n2 == -1, w . n2 == -0.0: bin 10, not 0
    'zero_normal': ((0, 0, 0), (0, 0, 0), (1, 0, 0), (0, 0, 1), (5, 5, 5)),                    # not refused: degenerate
    'zero_normal_swap': ((0, 0, 0), (0, 0, 0), (1, 0, 0), (1, 0, 0), (5, 5, 5)),               # swapped, then dp parallel to the normal
}
PAIR_RADIUS = 2.0


def pair_edge(name):
    p1, n1, p2, n2, want = PAIR_EDGES[name]
    return np.array([p1, p2], np.float64), np.array([n1, n2], np.float64), want


def _unit(g, n):
    v = g.standard_normal((n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


CLUSTER_SIZES = (1, 2, 64, 65, 66, 301)        # rows with 0, 1, 63, 64, 65 and 300 neighbours


@functools.lru_cache(None)
def edge_clouds():
    """name -> (points, normals, radius, max_nn)"""
    g = np.random.default_rng(21)
    out = {}
    for name in PAIR_EDGES:
        p, nr, _ = pair_edge(name)
        out['pair_' + name] = (p, nr, PAIR_RADIUS, None)
    # tight clusters far apart: every row of a cluster of s points has s - 1 neighbours (the lane stride of 64 and the tile of the loops)
    p = np.concatenate([10.0 * k + g.uniform(0, 0.1, (s, 3)) for k, s in enumerate(CLUSTER_SIZES)])
    shuffle = g.permutation(len(p))
    out['clusters'] = (p[shuffle], _unit(g, len(p)), 0.25, None)
    # a cloud whose ball holds the whole cloud, and a cloud of isolated points
    out['dense'] = (g.uniform(0, 0.1, (200, 3)), _unit(g, 200), 0.25, None)
    out['isolated'] = (np.stack(np.meshgrid(np.arange(4.0), np.arange(4.0), np.arange(3.0), indexing='ij'), -1).reshape(-1, 3), _unit(g, 48), 0.25, None)
    # an isolated point beside a pair: a zero row and two rows with one neighbour
    out['one_neighbour'] = (np.array([[0.0, 0, 0], [0.1, 0.05, 0], [5.0, 5, 5]]), _unit(g, 3), 0.25, None)
    small = g.uniform(0, 1, (40, 3))
    out['knn_1'] = (small, _unit(g, 40), None, 1)                        # the row itself alone: zero rows
    out['knn_2'] = (small, _unit(g, 40), None, 2)
    big = g.uniform(0, 1, (150, 3))
    out['knn_64'] = (big, _unit(g, 150), None, 64)
    out['knn_above_n'] = (small[:9], _unit(g, 9), None, 33)               # n < K
    out['hybrid'] = (big, _unit(g, 150), 0.3, 20)
    dup = g.uniform(0, 1, (30, 3))
    out['duplicates'] = (np.concatenate([dup, dup[:12]]), _unit(g, 42), 0.5, None)
    out['duplicates_knn'] = (np.tile(np.array([[0.25, -0.5, 0.125]]), (70, 1)), _unit(g, 70), None, 64)   # rows 64.. are not in their own result
    for n in (0, 1, 2, R - 1, R, R + 1):
        out['n%d' % n] = (g.uniform(0, 0.3, (n, 3)), _unit(g, n), 0.25, None)
    for v in out.values():
        v[0].setflags(write=False), v[1].setflags(write=False)
    return out


# ---- the library's host entries (the __host__ __device__ text of the kernels, no GPU) -----------------------------------------------------------
def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def host_list(points, radius=None, max_nn=None):
    """The neighbour list of one cloud from se3_debug_pair_ball_host (radius alone) or se3_debug_knn_host (max_nn, masked by the radius):
    (row_offsets (n + 1,) int64, pairs (total, 2) int64), neighbours ascending within a row."""
    from se3et_amd import _lib as L
    p = np.ascontiguousarray(points).reshape(-1, 3)
    assert p.dtype in (np.float32, np.float64)
    n, elem = len(p), int(p.dtype == np.float64)
    q = p if n else np.zeros((1, 3), p.dtype)
    if max_nn is None:
        eye = np.eye(4)
        counts, total = np.zeros(max(n, 1), np.int64), np.zeros(1, np.int64)
        L.check(L.lib().se3_debug_pair_ball_host(_ptr(q), n, _ptr(q), n, elem, _ptr(eye), float(radius), _ptr(counts), None, 0, _ptr(total)),
                'se3_debug_pair_ball_host')
        pairs = np.zeros((max(int(total[0]), 1), 2), np.int64)
        L.check(L.lib().se3_debug_pair_ball_host(_ptr(q), n, _ptr(q), n, elem, _ptr(eye), float(radius), _ptr(counts), _ptr(pairs), int(total[0]),
                                                 _ptr(total)), 'se3_debug_pair_ball_host')
        return np.concatenate([[0], np.cumsum(counts[:n])]).astype(np.int64), pairs[:int(total[0])]
    idx, d2 = np.full((max(n, 1), max_nn), -1, np.int64), np.full((max(n, 1), max_nn), np.inf)
    L.check(L.lib().se3_debug_knn_host(_ptr(q), n, _ptr(q), n, elem, int(max_nn), _ptr(idx), _ptr(d2)), 'se3_debug_knn_host')
    idx, d2 = idx[:n], d2[:n]
    keep = idx >= 0
    if radius is not None:
        keep &= d2 < np.float64(radius) * np.float64(radius)
    rows = [np.sort(idx[i][keep[i]]) for i in range(n)]
    ro = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    pairs = np.stack([np.repeat(np.arange(n), [len(r) for r in rows]), np.concatenate(rows + [np.zeros(0, np.int64)])], 1).astype(np.int64)
    return ro, np.ascontiguousarray(pairs.reshape(-1, 2))


def host_fpfh(points, normals, radius=None, max_nn=None):
    """se3_debug_fpfh_host on the list of host_list: (spfh (n, 33), fpfh (n, 33), status)."""
    from se3et_amd import _lib as L
    if radius is None and max_nn is None:
        raise ValueError('neither radius nor max_nn')
    p, nr = np.ascontiguousarray(points).reshape(-1, 3), np.ascontiguousarray(normals).reshape(-1, 3)
    n = len(p)
    ro, pairs = host_list(p, radius, max_nn)
    spfh, fpfh = np.full((max(n, 1), twin.DIM), -7.0), np.full((max(n, 1), twin.DIM), -7.0)
    status = np.full(1, -1, np.int32)
    some = np.zeros((1, 3), np.float64)
    L.check(L.lib().se3_debug_fpfh_host(_ptr(p if n else some), _ptr(nr if n else some), n, int(p.dtype == np.float64), int(nr.dtype == np.float64),
                                        _ptr(ro), _ptr(pairs if len(pairs) else np.zeros((1, 2), np.int64)), len(pairs), _ptr(spfh), _ptr(fpfh),
                                        _ptr(status)), 'se3_debug_fpfh_host')
    return spfh[:n], fpfh[:n], int(status[0])


def host_sectors():
    from se3et_amd import _lib as L
    out = np.zeros((10, 2))
    L.check(L.lib().se3_debug_fpfh_sectors_host(_ptr(out)), 'se3_debug_fpfh_sectors_host')
    return out
